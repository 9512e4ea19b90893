"""The attribute head of detector pre-training (the surface of AttrHead in the reference's models/detection/heads.py:33-51; its
class / box heads live in DetectionModule.detection_head here).  Visual Genome annotates objects with attributes; the head predicts
them from a query's hidden state and the embedding of the object class the detector currently prefers for it."""
from torch import nn

from grit_amd.ops.det_attr import attr_embed_cat
from grit_amd.ops.linear import Linear, linear_relu_dropout, mark_single_use


class AttrHead(nn.Module):
    """forward(obj_h [B, Q, d], pred_logits [B, Q, K]) -> {'attr_logits': [B, Q, A]}:
    attr_linear2(relu(attr_linear1(cat[obj_h, od_cls_embed(argmax sigmoid(pred_logits))]))).  State-dict keys as the reference's:
    od_cls_embed.weight, attr_linear1.{weight, bias}, attr_linear2.{weight, bias}.

    On the device the label, the embedding lookup and the concatenation are ONE launch (grit_attr_embed_cat), the embedding's
    gradient one more without atomics (grit_attr_embed_grad, grit_amd/ops/det_attr.py); the two Linears are the project's own
    (grit_amd/ops/linear.py).  No gradient reaches pred_logits, as in the reference.  CPU tensors run the host form."""

    def __init__(self, d_model, num_attr_classes, num_od_classes):
        super().__init__()
        self.od_cls_embed = nn.Embedding(num_od_classes, d_model)
        self.attr_linear1 = Linear(d_model + d_model, d_model)
        self.attr_linear2 = Linear(d_model, num_attr_classes)
        mark_single_use(self.attr_linear1, self.attr_linear2)  # once per forward: their weight gradients may wait for the grouped launch

    def forward(self, obj_h, pred_logits):
        if pred_logits.shape[-1] != self.od_cls_embed.num_embeddings:
            raise ValueError("AttrHead: %d class logits for an embedding of %d classes" % (pred_logits.shape[-1], self.od_cls_embed.num_embeddings))
        attr, _ = attr_embed_cat(obj_h, pred_logits, self.od_cls_embed.weight)
        # ReLU in attr_linear1's epilogue where the short-map tile takes the shape (p = 0: no dropout in this head)
        return {'attr_logits': self.attr_linear2(linear_relu_dropout(attr, self.attr_linear1, 0.0))}
