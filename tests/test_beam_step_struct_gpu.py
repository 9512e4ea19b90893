"""grit_beam_step through its argument struct, for what five positional entry points could not express: combinations that are
refused (forced words with groups, forced words without new_met, nine maps) leave the outputs untouched; a zero-initialised struct
with only the plain fields is the plain step; with no rule set t and history are not read; one group is the plain step whatever
the penalty; one map through `beam_step_mean` is `beam_step`; and the plain and mean fronts launch an evenly spaced view in place.
Every comparison is bit-equality with `beam_step` on the same tensors."""
import ctypes

import pytest
import torch

from tests.helpers import BEAM_STEP_OUTPUTS, beam_step_raw

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, V, K, EOS = 2, 1003, 6, 3
CURS = (1, K)  # the first step (one source row, eight slices a row) and a later one (K rows, two slices a row)


def state(cur, seed=1, n_maps=1, pad=0):
    """maps [B, cur, V] (views of [B, cur, V + pad] tensors), running scores, and at a later step a mask and previous words
    with one finished beam an image"""
    gen = torch.Generator(device=DEV).manual_seed(seed + cur)
    maps = [torch.log_softmax(3 * torch.randn(B, cur, V + pad, device=DEV, generator=gen), -1)[:, :, :V] for _ in range(n_maps)]
    seq_lp = -torch.rand(B, cur, 1, device=DEV, generator=gen) * 2
    if cur == 1:
        return maps, seq_lp, None, None
    prev = torch.full((B * cur, 1), 9, dtype=torch.int64, device=DEV)
    prev[2::cur] = EOS
    return maps, seq_lp, torch.ones(B, cur, 1, device=DEV), prev


def raw(maps, seq_lp, seq_mask, prev, **fields):
    """the status and the six outputs (pre-filled with -7; new_met is handed over only where `fields` says so)"""
    from grit_amd import lib
    cur = maps[0].shape[1]
    out = [torch.full((B, K), -7, dtype=torch.int64, device=DEV), torch.full((B, K), -7, dtype=torch.int64, device=DEV)] + \
        [torch.full((B, K, 1), -7.0, device=DEV) for _ in range(3)] + [torch.full((B, K), -7, dtype=torch.int32, device=DEV)]
    nbytes = lib.load().grit_beam_step_workspace(B, cur, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    given = dict(maps=maps, ld=maps[0].stride(1), seq_logprob=seq_lp, seq_mask=seq_mask, prev_words=prev, eos=EOS,
                 first_step=int(prev is None), B=B, cur_beam=cur, V=V, k=K, workspace=ws, workspace_bytes=nbytes,
                 **dict(zip(BEAM_STEP_OUTPUTS[:5], out)))
    if fields.pop("with_new_met", False):
        given["new_met"] = out[5]
    given.update(fields)
    return beam_step_raw(**given), out


def untouched(out):
    return all((o == -7).all() for o in out)


def assert_same(got, want, tag=""):
    for n, a, b in zip(BEAM_STEP_OUTPUTS, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, n)
        assert torch.equal(a, b), (tag, n)
        if a.dtype == torch.float32:  # signed zeros included
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (tag, n)


@pytest.mark.parametrize("cur", CURS)
def test_refused_combinations_write_nothing(cur):
    from grit_amd import lib
    maps, seq_lp, seq_mask, prev = state(cur)
    fw = torch.full((B, 2, 2), 7, dtype=torch.int64, device=DEV)
    forced = dict(force_words=fw, n_sets=2, n_words=2)
    st, out = raw(maps, seq_lp, seq_mask, prev, groups=2, with_new_met=True, **forced)
    assert st == lib.ERR_BAD_ARG and untouched(out)  # forced words have no groups
    st, out = raw(maps, seq_lp, seq_mask, prev, **forced)
    assert st == lib.ERR_BAD_ARG and untouched(out)  # new_met == NULL
    st, out = raw(maps * 9, seq_lp, seq_mask, prev)
    assert st == lib.ERR_UNSUPPORTED and untouched(out)  # n_maps = 9


@pytest.mark.parametrize("cur", CURS)
def test_plain_fields_alone_are_the_plain_step(cur):
    """... and so are the struct with t = 65 and no history while no rule is set, and one group under a penalty"""
    from grit_amd import lib
    from grit_amd.ops.beam import beam_step
    maps, seq_lp, seq_mask, prev = state(cur)
    want = beam_step(maps[0], seq_lp, seq_mask, prev, EOS, K)
    for tag, fields in (("plain", {}), ("t is not read", dict(t=65, history=None)), ("one group", dict(groups=1, diversity=0.5))):
        st, out = raw(maps, seq_lp, seq_mask, prev, **fields)
        assert st == lib.OK, tag
        assert_same(out[:5], want, tag)
        assert (out[5] == -7).all(), tag  # new_met is not written


@pytest.mark.parametrize("cur", CURS)
def test_one_map_through_the_mean_front_is_the_plain_step(cur):
    from grit_amd.ops.beam import beam_step, beam_step_mean
    maps, *rest = state(cur, seed=5)
    for a, b in zip(beam_step_mean(maps, *rest, EOS, K), beam_step(maps[0], *rest, EOS, K)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cur", CURS)
def test_spaced_maps_are_launched_in_place(cur, monkeypatch):
    """rows V + 5 floats apart: the plain and the mean front hand over the view's own address and its row stride"""
    from grit_amd import lib
    from grit_amd.ops.beam import beam_step, beam_step_mean
    maps, *rest = state(cur, seed=9, n_maps=2, pad=5)
    assert not maps[0].is_contiguous() and maps[0].stride(1) == V + 5
    dense = [m.contiguous() for m in maps]
    want = beam_step(dense[0], *rest, EOS, K), beam_step_mean(dense[:1], *rest, EOS, K), beam_step_mean(dense, *rest, EOS, K)
    real, seen = lib.load(), []

    class Spy(object):
        def __getattr__(self, name):
            return getattr(real, name)

        def grit_beam_step(self, args, stream):
            a = args._obj
            table = ctypes.cast(a.maps, ctypes.POINTER(ctypes.c_void_p))
            seen.append(([table[m] for m in range(a.n_maps)], a.ld))
            return real.grit_beam_step(args, stream)

    monkeypatch.setattr(lib, "load", lambda: Spy())
    got = beam_step(maps[0], *rest, EOS, K), beam_step_mean(maps[:1], *rest, EOS, K), beam_step_mean(maps, *rest, EOS, K)
    assert seen == [([maps[0].data_ptr()], V + 5)] * 2 + [([m.data_ptr() for m in maps], V + 5)]
    for g, w, tag in zip(got, want, ("plain", "mean of one", "mean of two")):
        assert_same(g, w, tag)
