"""The attribute head of detector pre-training on the device (grit_attr_embed_{cat,grad}, grit_det_attr_{fwd,bwd}_f32,
include/grit_hip.h): the head's front -- label of every query, class embedding, concatenation -- as one launch with a one-launch,
atomic-free gradient of the embedding table, and the weighted attribute loss of the matched queries as one autograd node next to the
set criterion's.  Each piece also has a host form, a plain torch composition of the same maths: what CPU tensors run, and what the
tests and tools/bench_det_attr.py compare the kernels with.

Nothing here reads a device value back.
"""
import torch

from grit_amd import lib as _lib

_p = _lib.ptr


# ---- host forms ------------------------------------------------------------------------------------------------------------------

def attr_labels_host(pred_logits):
    """[..., K] -> [...] int64: the first index of the largest fp32 sigmoid (reference heads.py:44-45).  The sigmoid saturates at
    1.0 from a logit of about 16.7, so this is not the argmax of the logits."""
    return torch.argmax(torch.sigmoid(pred_logits.float()), dim=-1)


def attr_embed_cat_host(obj_h, pred_logits, weight):
    """obj_h [..., d], pred_logits [..., K], weight [K, d] -> (cat[obj_h, weight[labels]] [..., 2 d], labels [...] int32)."""
    labels = attr_labels_host(pred_logits)
    return torch.cat([obj_h, weight[labels].to(obj_h.dtype)], dim=-1), labels.to(torch.int32)


def attr_embed_grad_host(dcat, labels, K):
    """The embedding table's gradient [K, d] from d(cat) [rows, 2 d] and labels [rows]: the right halves of the rows summed per class."""
    d = dcat.shape[-1] // 2
    part = dcat.reshape(-1, 2 * d)[:, d:]
    return torch.zeros(K, d, dtype=part.dtype, device=dcat.device).index_add_(0, labels.reshape(-1).to(torch.int64), part)


def attr_loss_host(attr_logits, attributes, offsets, has_attr, match_t):
    """The reference's weighted_attr_loss (od_losses.py:141-177) without its host-side index lists: attr_logits [B, Q, A],
    attributes [sum T + 1, A] (0 / 1), offsets [B + 1], has_attr [B] bool, match_t [B, Q] (target of each query or -1) ->
    the 0-d loss in attr_logits' dtype.  Differentiable by autograd; no data-dependent shape, so no synchronisation."""
    x = attr_logits
    t = match_t.to(torch.int64)
    sel = (has_attr.to(torch.bool)[:, None] & (t >= 0)).to(x.dtype)[..., None]  # [B, Q, 1]
    rows = offsets[:-1].to(torch.int64)[:, None] + t.clamp(min=0)
    y = (attributes[rows] != 0).to(x.dtype)  # [B, Q, A]
    bce = x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    on, off = y * sel, (1 - y) * sel
    n1, n0 = on.sum(), off.sum()
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    inside = torch.where(n1 > 0, (bce * on).sum() / n1.clamp(min=1), zero)
    outside = torch.where(n0 > 0, (bce * off).sum() / n0.clamp(min=1), zero)
    return inside + outside


# ---- the head's front ------------------------------------------------------------------------------------------------------------

def _io_dtype(t, what):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.GritHipError("%s: fp32 or bf16, got %s" % (what, t.dtype))
    return t.dtype == torch.bfloat16


def embed_cat(obj_h, pred_logits, weight):
    """grit_attr_embed_cat on device tensors, no autograd: obj_h [rows, d], pred_logits [rows, K], weight [K, d] ->
    (out [rows, 2 d], labels [rows] int32)."""
    _lib.require_device(obj_h, pred_logits, weight)
    rows, d = obj_h.shape
    K = weight.shape[0]
    if obj_h.dtype != weight.dtype or tuple(weight.shape) != (K, d) or tuple(pred_logits.shape) != (rows, K):
        raise _lib.GritHipError("attr embed cat: obj_h [rows, d] and weight [K, d] of one dtype and logits [rows, K], got %s %s, %s %s, %s"
                                % (tuple(obj_h.shape), obj_h.dtype, tuple(weight.shape), weight.dtype, tuple(pred_logits.shape)))
    bf16, logits_bf16 = _io_dtype(obj_h, "attr embed cat"), _io_dtype(pred_logits, "attr embed cat (logits)")
    obj_h = obj_h if obj_h.is_contiguous() else obj_h.contiguous()
    pred_logits = pred_logits if pred_logits.is_contiguous() else pred_logits.contiguous()
    weight = weight if weight.is_contiguous() else weight.contiguous()
    out = torch.empty((rows, 2 * d), dtype=obj_h.dtype, device=obj_h.device)
    labels = torch.empty((rows,), dtype=torch.int32, device=obj_h.device)
    lib = _lib.load()
    with _lib.device_guard(obj_h.device):
        st = lib.grit_attr_embed_cat(_p(obj_h), _p(pred_logits), _p(weight), _p(out), _p(labels), rows, K, d, int(bf16), int(logits_bf16),
                                     _lib.current_stream_ptr())
    _lib.check(st, "grit_attr_embed_cat")
    return out, labels


def embed_grad(dcat, labels, K, out=None):
    """grit_attr_embed_grad: dcat [rows, 2 d] (fp32 or bf16, rows contiguous), labels [rows] int32 -> d weight [K, d] in dcat's
    dtype.  Every element of the result is written."""
    _lib.require_device(dcat, labels)
    rows, two_d = dcat.shape
    d = two_d // 2
    if two_d != 2 * d or labels.dtype != torch.int32 or labels.numel() != rows or not labels.is_contiguous():
        raise _lib.GritHipError("attr embed grad: dcat [rows, 2 d] and labels [rows] int32")
    bf16 = _io_dtype(dcat, "attr embed grad")
    dcat = dcat if dcat.is_contiguous() else dcat.contiguous()
    if out is None:
        out = torch.empty((K, d), dtype=dcat.dtype, device=dcat.device)
    elif tuple(out.shape) != (K, d) or out.dtype != dcat.dtype or not out.is_contiguous() or not out.is_cuda:
        raise _lib.GritHipError("attr embed grad: out must be a contiguous [K, d] device tensor of dcat's dtype")
    lib = _lib.load()
    with _lib.device_guard(dcat.device):
        st = lib.grit_attr_embed_grad(_p(dcat), _p(labels), _p(out), rows, K, d, two_d, d, int(bf16), _lib.current_stream_ptr())
    _lib.check(st, "grit_attr_embed_grad")
    return out


class _EmbedCatFn(torch.autograd.Function):
    """[obj_h | weight[label]] and the labels.  d obj_h is the left half of the buffer's gradient (a view), d weight is
    grit_attr_embed_grad; the logits get none (the reference's argmax passes none either)."""

    @staticmethod
    def forward(ctx, obj_h, pred_logits, weight):
        d = obj_h.shape[-1]
        out, labels = embed_cat(obj_h.reshape(-1, d), pred_logits.reshape(-1, pred_logits.shape[-1]), weight)
        ctx.save_for_backward(labels)
        ctx.K, ctx.lead = weight.shape[0], tuple(obj_h.shape[:-1])
        labels = labels.view(ctx.lead)
        ctx.mark_non_differentiable(labels)
        return out.view(ctx.lead + (2 * d,)), labels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dcat, _):
        labels, = ctx.saved_tensors
        d = dcat.shape[-1] // 2
        dcat = dcat if dcat.is_contiguous() else dcat.contiguous()
        dobj = dcat[..., :d] if ctx.needs_input_grad[0] else None
        dweight = embed_grad(dcat.view(-1, 2 * d), labels, ctx.K) if ctx.needs_input_grad[2] else None
        return dobj, None, dweight


def attr_embed_cat(obj_h, pred_logits, weight):
    """obj_h [..., d], pred_logits [..., K], weight [K, d] -> (cat [..., 2 d], labels [...] int32).  Device tensors go through
    grit_attr_embed_cat (one launch), CPU tensors through the host form."""
    if not obj_h.is_cuda:
        return attr_embed_cat_host(obj_h, pred_logits, weight)
    return _EmbedCatFn.apply(obj_h, pred_logits, weight)


# ---- the loss --------------------------------------------------------------------------------------------------------------------

class _AttrLossFn(torch.autograd.Function):
    """loss_attr of grit_det_attr_fwd_f32; the forward leaves (N1, N0) on the device for the one-launch backward."""

    @staticmethod
    def forward(ctx, attr_logits, match_t, packed):
        B, Q, A = attr_logits.shape
        dev = attr_logits.device
        chunks = (Q + _lib.DET_LOSS_ROWS - 1) // _lib.DET_LOSS_ROWS
        partials = torch.empty((B * chunks, 2), dtype=torch.float64, device=dev)
        counts = torch.empty((B * chunks, 2), dtype=torch.int64, device=dev)
        ticket = torch.empty(1, dtype=torch.int32, device=dev)  # this call's own, zeroed by the entry point
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        lib = _lib.load()
        with _lib.device_guard(dev):
            st = lib.grit_det_attr_fwd_f32(_p(attr_logits), _p(packed.attributes), _p(packed.offsets), _p(packed.has_attr), _p(match_t),
                                           B, Q, A, _p(partials), _p(counts), _p(ticket), _p(loss), _p(totals), _lib.current_stream_ptr())
        _lib.check(st, "grit_det_attr_fwd_f32")
        ctx.save_for_backward(attr_logits, match_t, totals)
        ctx.packed = packed
        return loss.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        attr_logits, match_t, totals = ctx.saved_tensors
        packed = ctx.packed
        B, Q, A = attr_logits.shape
        upstream = grad_out.to(torch.float32).reshape(1)
        upstream = upstream if upstream.is_contiguous() else upstream.contiguous()
        dlogits = torch.empty_like(attr_logits)
        lib = _lib.load()
        with _lib.device_guard(attr_logits.device):
            st = lib.grit_det_attr_bwd_f32(_p(attr_logits), _p(packed.attributes), _p(packed.offsets), _p(packed.has_attr), _p(match_t),
                                           B, Q, A, _p(totals), _p(upstream), _p(dlogits), _lib.current_stream_ptr())
        _lib.check(st, "grit_det_attr_bwd_f32")
        return dlogits, None, None


def attr_loss(attr_logits, match_t, packed):
    """attr_logits [B, Q, A] fp32, match_t [B, Q] int32 (the last layer's slab of det_loss.match), packed: det_loss.pack_targets
    of targets that may carry 'attributes' / 'has_attr' -> the 0-d fp32 loss_attr (differentiable in attr_logits)."""
    _lib.require_device(attr_logits, match_t)
    if attr_logits.dim() != 3 or attr_logits.dtype != torch.float32:
        raise _lib.GritHipError("det attr loss: attr_logits must be [B, Q, A] fp32 (cast the head's output with .float()), got %s %s"
                                % (tuple(attr_logits.shape), attr_logits.dtype))
    B, Q, A = attr_logits.shape
    if B != len(packed):
        raise _lib.GritHipError("det attr loss: %d images in attr_logits, %d target entries" % (B, len(packed)))
    if packed.attributes is None or packed.has_attr is None:
        packed.add_attributes(A)
    if packed.attributes.shape[1] != A:
        raise _lib.GritHipError("det attr loss: the targets carry %d attribute classes, attr_logits %d" % (packed.attributes.shape[1], A))
    if packed.attributes.device != attr_logits.device:
        raise _lib.GritHipError("det attr loss: outputs on %s, targets on %s" % (attr_logits.device, packed.attributes.device))
    if match_t.dtype != torch.int32 or tuple(match_t.shape) != (B, Q) or not match_t.is_contiguous():
        raise _lib.GritHipError("det attr loss: match_t must be a contiguous [B, Q] int32 tensor")
    attr_logits = attr_logits if attr_logits.is_contiguous() else attr_logits.contiguous()
    return _AttrLossFn.apply(attr_logits, match_t, packed)
