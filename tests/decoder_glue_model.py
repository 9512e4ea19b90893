"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  Plain references of the ten small kernels that hold the two decoders together
(grit_amd/csrc/decoder.hip: gate_pack, gate_fuse, kv_append, decode_step_inputs; grit_amd/csrc/glue.hip: msda_geometry_fwd / _bwd,
box_refine, relu_dropout, gate_bwd_a / _b), written from the comment blocks at the top of each kernel, and builders of the inputs on
which such kernels go wrong.

Every arithmetic reference computes in float64 whatever the dtype of its inputs (the inputs are taken as they are: already rounded
to the kernel's dtype, so input rounding is no part of the error), spells out its own softmax, sigmoid and clamps instead of
calling torch's, and works on whatever device its inputs live on (torch tensor operations only; no kernel of this project).
tests/test_decoder_glue_model_cpu.py checks each of them against torch's composed form and torch.autograd in float64;
tests/test_decoder_glue_edges_gpu.py then holds the kernels to them.
"""
import numpy as np
import torch

SQRT2 = float(np.sqrt(2.0))
C_F32 = float(np.float32(1.0) / np.float32(np.sqrt(2)))  # what the kernels (and torch, for `/ np.sqrt(2)` in fp32) multiply by
GATE_VALUES = (0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, float("inf"), float("-inf"))
BOX_REF_VALUES = (-0.3, 0.0, 1e-5, 0.5, 1 - 1e-5, 1.0, 1.7)  # both clamps, the edges of both eps branches
EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------ MSDA geometry

def softmax64(logits):
    x = logits.double()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def _wh64(shapes, device):
    """[1, 1, 1, L, 1, 2] (W_l, H_l): spatial_shapes rows are (H, W); x is divided by W."""
    return torch.stack([shapes[:, 1], shapes[:, 0]], -1).double().to(device)[None, None, None, :, None, :]


def geometry(offsets, logits, ref, shapes, M, L, P):
    """offsets [N, Lq, M*L*P*2], logits [N, Lq, M*L*P], ref [N, Lq, L, 2|4], shapes [L, 2] -> loc [N, Lq, M, L, P, 2],
    aw [N, Lq, M, L, P] in float64.  4-d: ref_xy + offset / P * ref_wh * 0.5; 2-d: ref_xy + offset / (W_l, H_l)."""
    N, Lq = offsets.shape[:2]
    o = offsets.double().view(N, Lq, M, L, P, 2)
    aw = softmax64(logits.view(N, Lq, M, L * P)).view(N, Lq, M, L, P)
    r = ref.double()[:, :, None, :, None, :2]
    if ref.shape[-1] == 4:
        loc = r + o / P * ref.double()[:, :, None, :, None, 2:] * 0.5
    else:
        loc = r + o / _wh64(shapes, o.device)
    return loc, aw


def geometry_grad(g_loc, g_aw, aw, ref, shapes, M, L, P):
    """Gradients of `geometry` w.r.t. offsets and logits: the offset scale, and a * (ga - sum(a * ga)) per (row, head)."""
    N, Lq = aw.shape[:2]
    a, ga = aw.double().view(N, Lq, M, L * P), g_aw.double().view(N, Lq, M, L * P)
    d_log = a * (ga - (a * ga).sum(-1, keepdim=True))
    if ref.shape[-1] == 4:  # d(ref_xy + offset / P * ref_wh * 0.5) / d offset
        d_off = g_loc.double() * 0.5 * ref.double()[:, :, None, :, None, 2:] / P
    else:
        d_off = g_loc.double() / _wh64(shapes, g_loc.device)
    return d_off.reshape(N, Lq, M * L * P * 2), d_log.reshape(N, Lq, M * L * P)


# --------------------------------------------------------------------------------------------------------------- box_refine

def sigmoid64(x):
    return 1.0 / (1.0 + torch.exp(-x.double()))


def inverse_sigmoid64(x, eps=EPS):
    """log(clamp(x, 0, 1).clamp(min eps) / (1 - clamp(x, 0, 1)).clamp(min eps)); the comparisons are written out, so a NaN goes
    through every one of them untouched, as it does through torch.clamp."""
    x = x.double()
    zero, one, e = torch.zeros_like(x), torch.ones_like(x), torch.full_like(x, eps)
    x = torch.where(x < 0, zero, torch.where(x > 1, one, x))
    num = torch.where(x < eps, e, x)
    den = torch.where(1 - x < eps, e, 1 - x)
    return torch.log(num / den)


def box_refine(delta, ref):
    """delta [..., 4], ref [..., 2|4] -> sigmoid(delta + inverse_sigmoid(ref)); 2-d references move the centre only."""
    v = delta.double().clone()
    k = ref.shape[-1]
    v[..., :k] = v[..., :k] + inverse_sigmoid64(ref)
    return sigmoid64(v)


# -------------------------------------------------------------------------------------------------------------- gated merge

def gate_pack(self_att, enc1, enc2, mask):
    """[R, d] x 3, mask [R] -> [2R, 2d]: rows (self_att, enc1 * mask) then rows (self_att, enc2 * mask), in the inputs' dtype."""
    m = mask.view(-1, 1)
    return torch.cat([torch.cat([self_att, enc1 * m], 1), torch.cat([self_att, enc2 * m], 1)], 0)


def gate_products(enc1, enc2, G, mask):
    """The two products whose sum the merge scales: (enc1 m) sigmoid(G[:R]), (enc2 m) sigmoid(G[R:]), float64."""
    R = enc1.shape[0]
    m = mask.double().view(-1, 1)
    return enc1.double() * m * sigmoid64(G[:R]), enc2.double() * m * sigmoid64(G[R:])


def gate_fuse(enc1, enc2, G, mask, c=1.0 / SQRT2):
    """enc* [R, d], G [2R, d] gate pre-activations, mask [R] -> ((e1 s(G1) + e2 s(G2)) * c) * m, float64."""
    p1, p2 = gate_products(enc1, enc2, G, mask)
    return ((p1 + p2) * c) * mask.double().view(-1, 1)


def gate_bwd_a(d_out, enc1, enc2, G, mask, c=1.0 / SQRT2):
    """dG [2R, d]: t = d_out m c;  dG_i = t (enc_i m) s(G_i) (1 - s(G_i))."""
    R = enc1.shape[0]
    m = mask.double().view(-1, 1)
    t = d_out.double() * m * c
    s1, s2 = sigmoid64(G[:R]), sigmoid64(G[R:])
    return torch.cat([t * (enc1.double() * m) * s1 * (1 - s1), t * (enc2.double() * m) * s2 * (1 - s2)], 0)


def gate_bwd_b(d_out, G, mask, dX, c=1.0 / SQRT2):
    """dX [2R, 2d] = dG @ W -> d_self = dX[r, :d] + dX[R + r, :d];  d_enc_i = (t s(G_i) + dX[(i - 1) R + r, d:]) m."""
    R, d = d_out.shape
    m = mask.double().view(-1, 1)
    t = d_out.double() * m * c
    x = dX.double()
    d_self = x[:R, :d] + x[R:, :d]
    return d_self, (t * sigmoid64(G[:R]) + x[:R, d:]) * m, (t * sigmoid64(G[R:]) + x[R:, d:]) * m


# ------------------------------------------------------------------------------------------------------------- dropout hash

def dropout_uniform(seed, n):
    """The uniform draw of keep_scale in glue.hip for elements 0 .. n - 1, float32 multiples of 2^-24 in [0, 1):
    z = i + seed * 0x9E3779B97F4A7C15 (mod 2^64); x = low32(z ^ (z >> 32)); murmur3 finaliser on x (mod 2^32);
    u = float32(x >> 8) * 2^-24.  `seed` is any Python integer, taken modulo 2^64."""
    k = np.uint64((int(seed) % (1 << 64)) * 0x9E3779B97F4A7C15 % (1 << 64))
    z = np.arange(n, dtype=np.uint64) + k  # array arithmetic wraps
    x = (z ^ (z >> np.uint64(32))).astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(seed, n, p):
    """NumPy model of keep_scale in glue.hip: element i of a tensor is KEPT iff this is True: u >= float32(p), equality keeps."""
    return dropout_uniform(seed, n) >= np.float32(p)


def seed_as_int64(seed):
    """A 64-bit seed as the two's-complement int64 a torch tensor can hold."""
    seed = int(seed) % (1 << 64)
    return seed - (1 << 64) if seed >= (1 << 63) else seed


# ------------------------------------------------------------------------------------------------- key / value cache, step inputs

def kv_append(old, src, new, B, cur, beam):
    """old [B * cur, t, d], src [B, beam] int64 or None (identity), new [B * beam, 1, d] -> [B * beam, t + 1, d]:
    out[(b, j)][:t] = old[(b, src[b][j])], out[(b, j)][t] = new[(b, j)]."""
    if src is None:
        rows = torch.arange(B * beam, device=new.device)
    else:
        rows = (torch.arange(B, device=src.device).view(B, 1) * cur + src.view(B, beam)).reshape(-1)
    return torch.cat([old[rows], new], 1)


def step_inputs(tokens, pad, word_emb, pos_emb, seq, old_mask):
    """tokens [R, 1] int64, seq [R] step counters BEFORE the step, old_mask [R, 1, 1, t] bool -> x [R, 1, d] in the tables' dtype,
    new_mask [R, 1, 1, t + 1] bool, mask_pad [R, 1, 1] in the tables' dtype, the advanced counters [R]."""
    tok = tokens.reshape(-1)
    pos = seq + 1
    x = word_emb[tok] + pos_emb[pos]
    mask_pad = (tok != pad).to(word_emb.dtype)
    new_mask = torch.cat([old_mask.bool(), (tok == pad).view(-1, 1, 1, 1)], -1)
    return x.unsqueeze(1), new_mask, mask_pad.view(-1, 1, 1), pos


# -------------------------------------------------------------------------------------------------------------- hard inputs

def gate_preactivations(rows, d, dtype, gen):
    """[rows, d]: every value of GATE_VALUES in turn, each element starting at a random place of the cycle."""
    vals = torch.tensor(GATE_VALUES, dtype=torch.float32)
    idx = torch.randint(0, len(GATE_VALUES), (rows, d), generator=gen)
    return vals[idx].to(dtype)


def gate_case(rows, d, dtype, gen, hard=True):
    """Inputs of the gated merge with what makes it go wrong: masked rows (every third row when there are several; a lone row is
    live), +-0 in enc1, enc2 = -enc1 with equal gates on a part of the elements (the two products cancel), saturated gates.
    Returns dict(self_att, enc1, enc2 [rows, d], mask [rows], G [2 rows, d]), CPU tensors of `dtype`."""
    s = torch.randn(rows, d, generator=gen).to(dtype)
    e1 = (torch.randn(rows, d, generator=gen) * 2).to(dtype)
    e2 = (torch.randn(rows, d, generator=gen) * 2).to(dtype)
    mask = torch.ones(rows)
    if rows > 1:
        mask[1::3] = 0
    if hard:
        G = gate_preactivations(2 * rows, d, dtype, gen)
    else:
        G = (torch.randn(2 * rows, d, generator=gen) * 3).to(dtype)
    kind = torch.randint(0, 8, (rows, d), generator=gen)
    e1 = torch.where(kind == 0, torch.zeros_like(e1), e1)
    e1 = torch.where(kind == 1, -torch.zeros_like(e1), e1)
    cancel = kind == 2
    e2 = torch.where(cancel, -e1, e2)
    G = torch.cat([G[:rows], torch.where(cancel, G[:rows], G[rows:])], 0)
    return dict(self_att=s, enc1=e1, enc2=e2, mask=mask.to(dtype), G=G)


def tie_tables(vocab, n_pos, d, dtype, gen):
    """Embedding tables for decode_step_inputs.  Column 0..2 of word row 0 / `vocab - 1` and of EVERY position row hold pairs
    whose bf16 sum is a rounding tie (256 + 1 -> 256, 258 + 1 -> 260, -256 - 1 -> -256: nearest even); exact in fp32."""
    word = torch.randn(vocab, d, generator=gen)
    pos = torch.randn(n_pos, d, generator=gen)
    ties = torch.tensor([256.0, 258.0, -256.0])[:min(3, d)]
    ones = torch.tensor([1.0, 1.0, -1.0])[:min(3, d)]
    word[0, :len(ties)] = ties
    word[vocab - 1, :len(ties)] = ties
    pos[:, :len(ones)] = ones
    return word.to(dtype), pos.to(dtype)


def logit_rows(kind, shape, LP, dtype, gen):
    """[..., LP] softmax inputs: random, all equal, one-hot (one +80, the rest -80), or random on a large common offset."""
    x = torch.randn(*shape, LP, generator=gen)
    if kind == "equal":
        x = torch.full_like(x, 0.75)
    elif kind == "onehot":
        hot = torch.randint(0, LP, shape, generator=gen)
        x = torch.full_like(x, -80.0).scatter_(-1, hot.unsqueeze(-1), 80.0)
    elif kind == "offset":
        x = x + (1e4 if dtype == torch.float32 else 16.0)
    elif kind != "random":
        raise ValueError(kind)
    return x.to(dtype)


def box_references(rows, ref_dim, gen):
    """[rows, ref_dim] float32 drawn from BOX_REF_VALUES, every value present when rows * ref_dim allows."""
    vals = torch.tensor(BOX_REF_VALUES, dtype=torch.float32)
    n = rows * ref_dim
    idx = torch.arange(len(vals)).repeat(n // len(vals) + 1)[:n]
    idx = idx[torch.randperm(n, generator=gen)]
    return vals[idx].view(rows, ref_dim)
