"""Top-level `datasets` package of the reference, served by grit_amd.datasets for the detector's modules (datasets.detection,
datasets.detection.metrics, datasets.detection.metrics.coco_eval, datasets.detection.metrics.vg_eval)."""
import importlib
import sys

_PREFIX = 'grit_amd.datasets'
for _sub in ('', '.detection', '.detection.transforms', '.detection.metrics', '.detection.metrics.coco_eval', '.detection.metrics.vg_eval'):
    importlib.import_module(_PREFIX + _sub)
for _name, _mod in list(sys.modules.items()):
    if _name == _PREFIX or _name.startswith(_PREFIX + '.'):
        sys.modules['datasets' + _name[len(_PREFIX):]] = _mod
