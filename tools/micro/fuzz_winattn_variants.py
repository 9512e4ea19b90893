"""Window attention forward + backward on 36 random geometries; prints a digest per geometry.  Run once per kernel variant
(GRIT_WINATTN_FWD_DMA / GRIT_WINATTN_BWD_DMA) and compare the lines: tests/test_winattn_gpu.py does.

    --mask   adds "mask ..." lines: shift-6 geometries called with the shift mask as an explicit mask (the register-staged forward and
             the explicit-mask backward kernels)
    --drop   adds "drop ..." lines: B >= 2 with drop-path factors that zero some images and a cotangent that is zero there (the
             kernels that skip the windows of dropped images)"""
import sys, torch, hashlib, random
sys.path.insert(0, ".")
from grit_amd.ops.window_attention import window_attention
random.seed(1)
geos = []
for _ in range(36):
    nH = random.choice([1, 2, 3, 4, 8, 16])
    geos.append((random.randint(1, 3), random.randint(5, 50), random.randint(5, 50), nH, random.choice([0, 6])))


def shift_mask(H, W, shift):
    """The additive mask of the rolled, padded map ([windows per image, 144, 144]: -100 between different regions), built as Swin does."""
    Hp, Wp = -(-H // 12) * 12, -(-W // 12) * 12
    img = torch.zeros(Hp, Wp)
    cuts = (slice(0, -12), slice(-12, -shift), slice(-shift, None))
    for i, hs in enumerate(cuts):
        for j, ws in enumerate(cuts):
            img[hs, ws] = 3 * i + j
    win = img.view(Hp // 12, 12, Wp // 12, 12).permute(0, 2, 1, 3).reshape(-1, 144)
    return ((win[:, None, :] != win[:, :, None]).float() * -100.0).cuda()


cases = [("", geo, False, ()) for geo in geos]
if "--mask" in sys.argv:
    cases += [("mask ", geo, True, ()) for geo in [(1, 13, 30, 2, 6), (2, 24, 24, 4, 6), (1, 40, 17, 1, 6), (3, 5, 50, 8, 6)]]
if "--drop" in sys.argv:
    cases += [("drop ", geo, False, drop) for geo, drop in [((4, 20, 20, 4, 6), (1,)), ((3, 13, 30, 2, 0), (0, 2)), ((2, 24, 36, 8, 6), (1,)),
                                                             ((5, 40, 7, 16, 6), (0, 1, 3))]]
out = []
for (tag, (B, H, W, nH, shift), masked, drop) in cases:
    g = torch.Generator().manual_seed(H * 100 + W)
    C = 32 * nH
    qkv = torch.randn(B, H * W, 3 * C, generator=g).bfloat16().cuda().requires_grad_(True)
    bias = (torch.randn(nH, 144, 144, generator=g) * 0.5).bfloat16().float().cuda().requires_grad_(True)  # bf16-representable: the DMA backward keeps the slab in bf16
    pad = (torch.randn(3 * C, generator=g) * 0.3).bfloat16().cuda().requires_grad_(True)
    cot = torch.randn(B, H * W, C, generator=g).bfloat16().cuda()
    row_scale = None
    if drop:
        row_scale = torch.full((B,), 1.25)
        row_scale[list(drop)] = 0.0
        row_scale = row_scale.cuda()
        cot[list(drop)] = 0
    o = window_attention(qkv, bias, pad, H, W, nH, 12, shift, 32**-0.5, mask=shift_mask(H, W, shift) if masked else None, row_scale=row_scale)
    o.backward(cot)
    torch.cuda.synchronize()
    h = hashlib.sha1(o.detach().float().cpu().numpy().tobytes()).hexdigest()[:12]
    hq = hashlib.sha1(qkv.grad.float().cpu().numpy().tobytes()).hexdigest()[:12]
    # (the added lines name their digests tag:fwd / tag:dqkv: readers of the 36 default lines select them by " fwd ")
    keys = (" fwd ", " dqkv ") if not tag else (" %s:fwd " % tag.strip(), " %s:dqkv " % tag.strip())
    out.append("%s%s%s%s%s%s dbias %.6e dpad %.6e" % (tag, (B, H, W, nH, shift), keys[0], h, keys[1], hq, bias.grad.double().abs().sum().item(), pad.grad.double().abs().sum().item()))
print("\n".join(out))
