"""Region-feature extractor of GRIT (Deformable-DETR style decoder) and the pieces of its pre-training: the Detector with its
class / box heads (detector.py), the attribute head (heads.py) and the matcher and set criterion (od_losses.py).  Mask losses and
the Visual Genome readers of the reference are out of scope."""
