"""Region-feature extractor of GRIT (Deformable-DETR style decoder) and the pieces of its pre-training: the Detector with its
class / box heads (detector.py) and the matcher and set criterion (od_losses.py).  Attribute heads, mask losses, the datasets and
the COCO-style evaluation of the reference are out of scope."""
