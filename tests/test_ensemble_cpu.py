"""models.caption.ensemble.Ensemble on the CPU (oracle ops injected) against fixture G16, made by the reference's own Ensemble
(tests/golden/make_ensemble_golden.py): the reference signatures, the refusals, and the eager ensemble beam search."""
import inspect

import numpy as np
import pytest
import torch

from tests.helpers import deterministic_fill_, load, oracle_ops, t


def g16_features(g):
    return {'gri_feat': t(g['gri_feat_q16']).float() / 16, 'gri_mask': t(g['gri_mask']),
            'reg_feat': t(g['reg_feat_q16']).float() / 16, 'reg_mask': t(g['reg_mask'])}


def g16_member(i, n_layers=2, **over):
    """Decoder side of G16's member i (no detector: the fixture decodes from cached features)."""
    from grit_amd.config import default_config
    from grit_amd.models.caption import Transformer
    cfg = default_config(**{'model.cap_generator.n_layers': n_layers, **over})
    return deterministic_fill_(Transformer(None, cfg), 'e%d.' % i).eval(), cfg


@pytest.fixture(scope="module")
def members():
    return [g16_member(i)[0] for i in range(3)]


def test_reference_module_path_and_signatures():
    import models.caption.ensemble as mod
    from grit_amd.models.caption.ensemble import Ensemble
    assert mod.Ensemble is Ensemble
    init = inspect.signature(Ensemble.__init__)
    assert list(init.parameters) == ['self', 'models', 'bos_idx', 'use_vis_feat', 'use_reg_feat', 'config']
    assert [init.parameters[n].default for n in ('bos_idx', 'use_vis_feat', 'use_reg_feat', 'config')] == [2, True, False, None]
    fwd = inspect.signature(Ensemble.forward)
    assert list(fwd.parameters) == ['self', 'samples', 'seq', 'use_beam_search', 'max_len', 'eos_idx', 'beam_size', 'out_size',
                                    'return_probs', 'kwargs']
    assert [fwd.parameters[n].default for n in ('use_beam_search', 'max_len', 'eos_idx', 'beam_size', 'out_size',
                                                 'return_probs')] == [False, 20, 3, 5, 1, False]


def test_refusals(members):
    from grit_amd.models.caption.ensemble import Ensemble
    a, b = members[0], members[1]
    with pytest.raises(NotImplementedError, match="teacher-forcing"):
        Ensemble([a, b])(g16_features(load("ensemble_g16.npz")), None)
    small, _ = g16_member(0, **{'model.vocab_size': 101})
    with pytest.raises(ValueError, match="vocabulary"):
        Ensemble([a, small])
    other_bos, _ = g16_member(1, **{'model.bos_idx': 4})
    with pytest.raises(ValueError, match="bos"):
        Ensemble([a, other_bos])
    with pytest.raises(ValueError, match="bos"):
        Ensemble([a, b], bos_idx=4)
    other_eos, _ = g16_member(1, **{'model.eos_idx': 5})
    with pytest.raises(ValueError, match="eos"):
        Ensemble([a, other_eos])
    half, _ = g16_member(1)
    half.to(torch.float64)
    with pytest.raises(ValueError, match="one device with one dtype"):
        Ensemble([a, half])
    ens = Ensemble([a, b])
    b.to(torch.float64)  # moved after construction: refused at the next call
    try:
        with pytest.raises(ValueError, match="one device with one dtype"):
            ens(g16_features(load("ensemble_g16.npz")), None, use_beam_search=True)
    finally:
        b.to(torch.float32)
    with pytest.raises(ValueError, match="at least one"):
        Ensemble([])


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("beam,out_size", [(1, 1), (5, 1), (5, 5)])
def test_eager_ensemble_matches_reference(members, K, beam, out_size):
    """Tokens bit-exact, log-probs at G7's tolerance; the members leave stateless and keep their own decode-graph caches."""
    from grit_amd.models.caption.ensemble import Ensemble
    g = load("ensemble_g16.npz")
    tag = 'k%d_b%d_o%d' % (K, beam, out_size)
    ens = Ensemble(members[:K]).eval()
    with oracle_ops(), torch.no_grad():
        tokens, lps = ens(g16_features(g), seq=None, use_beam_search=True, max_len=20, eos_idx=3, beam_size=beam,
                          out_size=out_size)
    assert tokens.dtype == torch.int64 and tokens.shape == g[tag + '_tokens'].shape
    np.testing.assert_array_equal(tokens.numpy(), g[tag + '_tokens'])
    np.testing.assert_allclose(lps.numpy(), g[tag + '_logprobs'], rtol=1e-3, atol=1e-3)
    for m in members[:K]:
        assert not m._is_stateful and m.gri_feat is None and m.cached_features is False and not m._decode_graphs


def test_return_probs_and_features_per_member(members):
    """return_probs gives the averaged word log-probabilities of every kept beam; a list of feature dicts (one per member) is
    the same as one shared dict."""
    from grit_amd.models.caption.ensemble import Ensemble
    g = load("ensemble_g16.npz")
    ens = Ensemble(members[:2]).eval()
    with oracle_ops(), torch.no_grad():
        tok, lp, all_lp = ens(g16_features(g), None, use_beam_search=True, beam_size=5, out_size=1, return_probs=True)
        tok2, lp2 = ens([g16_features(g), g16_features(g)], None, use_beam_search=True, beam_size=5, out_size=1)
    np.testing.assert_array_equal(tok.numpy(), g['k2_b5_o1_tokens'])
    np.testing.assert_array_equal(tok2.numpy(), tok.numpy())
    np.testing.assert_array_equal(lp2.numpy(), lp.numpy())
    assert all_lp.shape == (3, 5, 20, 10201) and bool((all_lp <= 0).all())  # a mean of log-softmax rows


def test_evaluate_metrics_takes_an_ensemble(members, tmp_path):
    """engine.caption_engine.evaluate_metrics drives an Ensemble like a Transformer (eval(), beam search of every batch);
    asking it to save a best checkpoint is refused before the evaluation: an Ensemble's state dict is no model checkpoint."""
    from grit_amd.config import default_config
    from grit_amd.engine.caption_engine import evaluate_metrics, save_checkpoint
    from grit_amd.models.caption.ensemble import Ensemble
    g = load("ensemble_g16.npz")
    cfg = default_config(**{'model.cap_generator.n_layers': 2})
    ens = Ensemble(members[:2]).train()
    with oracle_ops():
        tokens, _ = evaluate_metrics(ens, None, [{'samples': g16_features(g)}], None, config=cfg)
    assert not ens.training and all(not m.training for m in members[:2])
    np.testing.assert_array_equal(tokens[0].numpy(), g['k2_b5_o1_tokens'])
    with pytest.raises(ValueError, match="no single-model checkpoint"):
        evaluate_metrics(ens, None, [{'samples': g16_features(g)}], None, config=cfg, best_cider=0.0, scorer=lambda a, b: {})
    with pytest.raises(ValueError, match="no single-model checkpoint"):
        save_checkpoint(ens, None, 0, [], (0, 0), filename=str(tmp_path / 'ens.pth'))
    assert not (tmp_path / 'ens.pth').exists()
