"""COCO-style evaluation of the detector (the reference's datasets/detection/metrics): box mAP from device-side matching."""
from .coco_eval import AnnotationIndex, BoxEval, CocoEvaluator, Params, accumulate_records, summarize_eval
