"""Evaluation of the detector (the reference's datasets/detection/metrics) from device-side matching: COCO-style box mAP
(coco_eval.py) and the Visual Genome protocol's object and attribute AP (vg_eval.py)."""
from .coco_eval import AnnotationIndex, BoxEval, CocoEvaluator, Params, accumulate_records, summarize_eval
from .vg_eval import VGEvaluator, accumulate_voc, voc_ap
