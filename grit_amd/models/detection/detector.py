"""The detector that is pre-trained on Visual Genome before any captioning run: Swin backbone -> input_proj -> DetectionModule ->
class / box heads.  The surface of the reference's models/detection/detector.py (Detector :22-74, build_detector :126-157) with its
state-dict keys (backbone.*, det_module.*, input_proj.*, and attr_head.* with model.has_attr_head)."""
import torch
import torch.nn.functional as F

from grit_amd.models.caption.detector import Detector as _FeatureDetector
from grit_amd.models.common.swin_model import swin_base_win7_384
from grit_amd.models.detection.det_module import build_det_module_with_config
from grit_amd.models.detection.heads import AttrHead
from grit_amd.models.detection.od_losses import PostProcess, PostProcessAttr, SetCriterion, build_matcher
from grit_amd.utils.misc import nested_tensor_from_tensor_list


class Detector(_FeatureDetector):
    """forward(samples) -> {'pred_logits', 'pred_boxes'[, 'aux_outputs']} of DetectionModule.detection_head.  The levels are
    projected as in the captioner's detector (GEMM + token-major GroupNorm into one flat map on the device).  With has_attr_head
    the model owns an AttrHead(hidden_dim, num_attr_classes, num_od_classes) and forward adds 'attr_logits' [B, Q, A], computed from
    the last decoder level's hidden states and class logits, in training and in evaluation."""

    def __init__(self, backbone, det_module, hidden_dim=256, has_attr_head=False, num_attr_classes=400, num_od_classes=1849):
        if has_attr_head and det_module is None:
            # (before anything touches `backbone`) the head reads hs[-1] and pred_logits, which only the detection module produces
            raise NotImplementedError("Detector: an attribute head needs a detection module (has_attr_head=True with det_module=None)")
        super().__init__(backbone, det_module=det_module, use_gri_feat=True, use_reg_feat=True, hidden_dim=hidden_dim)
        self.has_attr_head = bool(has_attr_head)
        if self.has_attr_head:
            self.attr_head = AttrHead(hidden_dim, num_attr_classes, num_od_classes)
        for proj in self.input_proj:
            torch.nn.init.xavier_uniform_(proj[0].weight, gain=1)
            torch.nn.init.constant_(proj[0].bias, 0)

    def forward(self, samples):
        if isinstance(samples, (list, tuple, torch.Tensor)):
            samples = nested_tensor_from_tensor_list(list(samples))
        x, mask = samples.tensors, samples.mask
        features = self.backbone(x)
        no_padding = getattr(samples, 'any_padding', None) is False
        if no_padding:
            masks = [mask.new_zeros((mask.shape[0],) + tuple(f.shape[-2:])) for f in features]
        else:
            masks = [F.interpolate(mask[None].float(), size=f.shape[-2:]).to(torch.bool)[0] for f in features]
        if x.is_cuda:
            flat, shapes = self.project_levels(features)
            hs, init_reference, inter_references = self.det_module(None, masks, no_padding=no_padding, src_flatten=flat, shapes=shapes)
        else:
            srcs = [proj(f) for proj, f in zip(self.input_proj, features)]
            hs, init_reference, inter_references = self.det_module(srcs, masks)
        outputs = self.det_module.detection_head(hs, init_reference, inter_references)
        if self.has_attr_head:
            outputs.update(self.attr_head(hs[-1], outputs['pred_logits']))
        return outputs


def build_weight_dict(det_cfg):
    """Loss name -> weight, with the `_i` entries of the auxiliary outputs and the `_enc` ones the reference lists as well."""
    loss_cfg = det_cfg.loss
    weight_dict = {'loss_ce': loss_cfg.cls_loss_coef, 'loss_bbox': loss_cfg.bbox_loss_coef, 'loss_giou': loss_cfg.giou_loss_coef,
                   'loss_attr': loss_cfg.attr_loss_coef}
    if det_cfg.aux_loss:
        base = dict(weight_dict)
        for suffix in ['_%d' % i for i in range(det_cfg.num_layers)] + ['_enc']:
            weight_dict.update({k + suffix: v for k, v in base.items()})
    return weight_dict


def build_detector(config):
    """(model, criterion, postprocessors) from a configuration with the keys of configs/detection/train_config.yaml.
    postprocessors: 'bbox' (PostProcess) and, when the model has the attribute head, 'attr' (PostProcessAttr)."""
    name = config.model.backbone.backbone_name
    if name != 'swin_base_win7_384_22k':
        raise ValueError('backbone %s not supported' % name)
    det_cfg = config.model.det_module
    backbone, _ = swin_base_win7_384(pretrained=getattr(config.model.backbone, 'pre_trained', None))
    if not hasattr(det_cfg, 'd_model'):  # the yaml names the decoder width reduced_dim, the module builder reads d_model
        det_cfg = type(det_cfg)(**{**vars(det_cfg), 'd_model': det_cfg.reduced_dim})
    model = Detector(backbone, build_det_module_with_config(det_cfg), hidden_dim=det_cfg.reduced_dim,
                     has_attr_head=bool(getattr(config.model, 'has_attr_head', False)),
                     num_attr_classes=getattr(config.model, 'num_attr_classes', 400), num_od_classes=det_cfg.num_classes)
    criterion = SetCriterion(det_cfg.num_classes, build_matcher(det_cfg.matcher), build_weight_dict(det_cfg),
                             ['labels', 'boxes', 'cardinality'], focal_alpha=det_cfg.loss.focal_alpha)
    postprocessors = {'bbox': PostProcess()}
    if model.has_attr_head:
        postprocessors['attr'] = PostProcessAttr()
    return model, criterion, postprocessors
