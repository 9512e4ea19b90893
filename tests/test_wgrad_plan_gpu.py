"""The launch plan of the weight-gradient host path (grit_amd/ops/linear.py): WHICH weight-gradient, column-sum and slab-sum launches a
backward pass plus finish_gradient_sync issues, in which order, with which problem sizes and slice counts.  Gradients within
tolerance do not pin that -- a host-side change can keep every number and still double the fp32 partial traffic -- so the ordered
record of four small passes is compared for equality with tests/golden/wgrad_launch_plan.json, and so is a bit-exact digest of
every parameter gradient that comes from the project's own kernels (no atomics on these routes: a pass repeats bit for bit).

`python -m tests.test_wgrad_plan_gpu [path]` writes the record (default: the golden file); the module imports only names that
have not changed since the record was taken, so it can be run unchanged in an older checkout to take the record there."""
import json
import os
import sys

import pytest
import torch

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_launch_plan.json")
DEV = "cuda"

_WGRAD = ("M", "N", "K", "splits", "ldy", "ldx", "rows_per_sample")
_GROUPED = {
    "grit_wgrad_tn_grouped": lambda j: dict({f: int(getattr(j, f)) for f in _WGRAD}, db_partial=bool(j.db_partial), row_scale=bool(j.row_scale)),
    "grit_colsum_grouped": lambda j: {f: int(getattr(j, f)) for f in ("M", "N", "slabs", "ld")},
    "grit_slab_sum_grouped": lambda j: dict({f: int(getattr(j, f)) for f in ("groups", "slabs", "n", "out_is_bf16")}, extra=bool(j.extra)),
}
_GROUPED["grit_wgrad_small_grouped"] = _GROUPED["grit_wgrad_tn_grouped"]
# ungrouped entry points: (name, position) of every integer argument, and of the optional pointers recorded as set / not set
_PLAIN = {
    "grit_wgrad_tn_rows": ((("ldy", 1), ("ldx", 3), ("M", 4), ("N", 5), ("K", 6), ("splits", 7), ("rows_per_sample", 11)),
                           (("db_partial", 9), ("row_scale", 10))),
    "grit_colsum": ((("M", 1), ("N", 2), ("is_bf16", 3), ("slabs", 4)), ()),
    "grit_slab_sum": ((("groups", 1), ("group_stride", 2), ("slabs", 3), ("n", 4), ("out_is_bf16", 6)), ()),
}


def _is_set(arg):
    return bool(getattr(arg, "value", arg))


class _Spies(object):
    """`with _Spies() as calls:` -- the entry points above on the loaded library append to `calls` and run."""

    def __enter__(self):
        from grit_amd.ops import linear as L
        self.lib = L._lib.load()
        self.real = {name: getattr(self.lib, name) for name in list(_GROUPED) + list(_PLAIN)}
        calls = []

        def grouped(name, real, fields):
            def spy(table, n, stream):
                calls.append({"call": name, "jobs": [fields(table[i]) for i in range(n)]})
                return real(table, n, stream)
            return spy

        def plain(name, real, ints, pointers):
            def spy(*args):
                rec = {"call": name}
                rec.update({f: int(args[i]) for f, i in ints})
                rec.update({f: _is_set(args[i]) for f, i in pointers})
                calls.append(rec)
                return real(*args)
            return spy

        for name, fields in _GROUPED.items():
            setattr(self.lib, name, grouped(name, self.real[name], fields))
        for name, (ints, pointers) in _PLAIN.items():
            setattr(self.lib, name, plain(name, self.real[name], ints, pointers))
        return calls

    def __exit__(self, *exc):
        for name, real in self.real.items():
            setattr(self.lib, name, real)


def _digest(grad):
    """Two int64 checksums of the gradient's bits (plain and position-weighted): equal tensors, equal digests."""
    if grad is None:
        return None
    bits = grad.detach().contiguous().view(torch.int16 if grad.element_size() == 2 else torch.int32).reshape(-1).to(torch.int64)
    weights = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 65521 + 1
    return [int(bits.sum().item()), int((bits * weights).sum().item())]


def _one_pass(net, inputs, loss_of, library=(), **ddp_args):
    """One forward + backward + finish_gradient_sync of `net` inside a gradient-bucket wrapper: (launch record, gradient digests).
    library: parameters whose gradient is the output of a library GEMM, left out of the digests -- the library picks its algorithm
    from the state of the process (grit_amd.tuning.load_tuned_gemms, once some earlier test has called it, switches TunableOp's
    solution table on), so those bits repeat from one fresh process to the next but not behind other tests."""
    from grit_amd.ddp import BucketedDataParallel
    for p in net.parameters():
        p.grad = None
    ddp = BucketedDataParallel(net, **ddp_args)
    out = ddp(*inputs)
    loss = loss_of(out)
    with _Spies() as calls:
        loss.backward()
        ddp.finish_gradient_sync()
    torch.cuda.synchronize()
    return {"plan": calls, "grads": {n: _digest(p.grad) for n, p in net.named_parameters() if n not in library}}


def _rand(*shape, grad=False):
    return torch.randn(*shape, device=DEV).bfloat16().requires_grad_(grad)


def _dot(y, cot):
    return (y.float() * cot.float()).sum()


def _short_maps():
    """The net of test_deferred_grouped_weight_gradients: the grouped long-kernel chunk, the small-kernel chunk (N = 128), the per-node path."""
    from grit_amd.ops import linear as L
    from grit_amd.ops.layer_norm import linear_add_layer_norm

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = L.Linear(512, 1024)
            self.b = torch.nn.Linear(1024, 512)
            self.c = L.Linear(512, 128)
            self.norm = torch.nn.LayerNorm(512)
            self.twice = L.Linear(512, 512)
            L.mark_single_use(self.a, self.b, self.c)

        def forward(self, x):
            h = torch.relu(self.a(x))
            x = linear_add_layer_norm(h, self.b, x, None, self.norm.weight, self.norm.bias, 1e-5, 0.0, True)[1]
            x = self.twice(torch.tanh(self.twice(x)))
            return x, self.c(x)

    torch.manual_seed(0)
    net = Net().to(DEV).bfloat16()
    x, cot, cot2 = _rand(8, 600, 512, grad=True), _rand(8, 600, 512), _rand(8, 600, 128)
    # (`twice` is not single-use: its weight gradient is two library GEMMs, torch.mm in weight_grad, summed by autograd)
    return {"short_maps": _one_pass(net, (x,), lambda o: _dot(o[0], cot) + _dot(o[1], cot2), library=("twice.weight",), bucket_mb=1)}


def _packed_in_projection():
    """The net of test_packed_in_projection_node: two row ranges of one packed parameter as two problems of the grouped launch."""
    from grit_amd.ops import linear as L

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mha = torch.nn.MultiheadAttention(512, 8)

        def forward(self, t, pos):
            return L.packed_in_proj(t + pos, t, self.mha.in_proj_weight, self.mha.in_proj_bias)

    torch.manual_seed(1)
    net = Net().to(DEV).bfloat16()
    with torch.no_grad():
        net.mha.in_proj_bias.normal_(0, 0.1)
    t, pos, c_qk, c_v = _rand(32, 150, 512, grad=True), _rand(32, 150, 512), _rand(32, 150, 1024), _rand(32, 150, 512)
    return {"packed_in_projection": _one_pass(net, (t, pos), lambda o: _dot(o[0], c_qk) + _dot(o[1], c_v), bucket_mb=1)}


def _parked():
    """The net of test_parked_weight_gradient_runs_in_its_partners_launch, with the partner and without it."""
    from grit_amd.ops import linear as L
    from grit_amd.ops.layer_norm import linear_add_layer_norm

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.qkv = L.Linear(512, 1536)
            self.proj = L.Linear(512, 512)
            self.norm = torch.nn.LayerNorm(512)
            L.mark_single_use(self.proj)
            L.park_weight_grad_for_partner(self.proj, self.qkv)
            self.skip_partner = False

        def forward(self, x):
            h = x if self.skip_partner else torch.tanh(self.qkv(x)[..., :512])
            s, n = linear_add_layer_norm(h, self.proj, x, None, self.norm.weight, self.norm.bias, self.norm.eps)
            return s + n

    torch.manual_seed(0)
    net = Net().to(DEV).bfloat16()
    x, cot = _rand(16, 1024, 512), _rand(16, 1024, 512)
    out = {}
    for name, skip in (("parked_with_partner", False), ("parked_without_partner", True)):
        net.skip_partner = skip
        out[name] = _one_pass(net, (x,), lambda y: _dot(y, cot), bucket_mb=64, tail_mb=0)
    return out


def _swin_mlp():
    """The backbone's Mlp through ops.mlp.mlp, single-use: both weight gradients in one grouped launch, bucket slots as outputs."""
    from grit_amd.models.common.swin_model import Mlp
    from grit_amd.ops import linear as L
    from grit_amd.ops.mlp import mlp

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mlp = Mlp(512, 2048)
            L.mark_single_use(self.mlp)

        def forward(self, x):
            return mlp(x, self.mlp)

    torch.manual_seed(0)
    net = Net().to(DEV).bfloat16()
    x, cot = _rand(16, 1024, 512, grad=True), _rand(16, 1024, 512)
    return {"swin_mlp": _one_pass(net, (x,), lambda y: _dot(y, cot), bucket_mb=64, tail_mb=0)}


def record():
    out = {}
    for passes in (_short_maps, _packed_in_projection, _parked, _swin_mlp):
        out.update(passes())
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_FILE) as f:
        want = json.load(f)
    return record(), want


@pytest.mark.gpu
def test_backward_issues_the_recorded_launches(recorded):
    """Same kernels, same order, same problem sizes, same slice counts as the record."""
    got, want = recorded
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        print(name, json.dumps(got[name]["plan"]))
        assert got[name]["plan"], name  # (a pass that launched nothing proves nothing)
        assert got[name]["plan"] == want[name]["plan"], name


@pytest.mark.gpu
def test_gradients_repeat_the_record_bit_for_bit(recorded):
    got, want = recorded
    differ = []
    for name in sorted(want):
        assert sorted(got[name]["grads"]) == sorted(want[name]["grads"]), name
        differ += [(name, param) for param, digest in want[name]["grads"].items() if got[name]["grads"][param] != digest]
    assert not differ


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN_FILE
    with open(path, "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
