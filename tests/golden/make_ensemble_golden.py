"""Fixture G16 (`ensemble_g16.npz`): the reference's `Ensemble` (models/caption/ensemble.py) beam-searching with two and three
reference `Transformer`s from small cached features.  Runs ONLY in the build container, on the CPU, like make_golden.py:

    python tests/golden/make_ensemble_golden.py

Members: 2-layer decoders (BASELINE config 1, as G7), every parameter filled by fill.py with the prefix 'e<i>.' of member i, so
the members differ.  Features: 3 images with G7's grid and region shapes (16 grid tokens of 1024, 150 regions of 512), seeded
normal values rounded to multiples of 1/16 and stored as int8 codes (`*_q16`: feature = code / 16); image 1's last 4 grid
tokens are masked (and zero).  Recorded per ensemble size K in {2, 3}: tokens and log-probs for (beam 1, out_size 1),
(beam 5, out_size 1) and (beam 5, out_size 5), and the per-step top-(beam + 1) candidate scores (the margin record).

The reference class does not run against the reference Transformer as it is: it reads `model.encoder`, `model.decoder` (with
the region features under the key 'det_feat'), `model.det_feat` and `config.model.decoder.decoder_name`.  THIS GENERATOR ALONE
gives each reference member those aliases before the run: `encoder` -> `grid_net`, `decoder` -> `cap_generator` with
'det_feat' renamed to 'reg_feat', the attribute `det_feat` -> the registered state `reg_feat` (so that it follows the beams),
and `config.model.decoder.decoder_name = 'parallel'`; the cached features are handed to it with the region features under
'det_feat' (recorded here as 'reg_feat').  Nothing else about the reference is changed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (import_reference, _cfg, _fill)


def _alias_for_reference_ensemble(model):
    cap = model.grid_net, model.cap_generator

    def decoder(it, vis, _gen=cap[1]):
        vis = dict(vis)
        if 'det_feat' in vis:
            vis['reg_feat'] = vis.pop('det_feat')
        return _gen(it, vis)

    # plain attributes (object.__setattr__): not registered as sub-modules, so no state is visited twice
    object.__setattr__(model, 'encoder', cap[0])
    object.__setattr__(model, 'decoder', decoder)
    model.__class__ = type('EnsembleMember', (type(model),), {
        'det_feat': property(lambda self: self.reg_feat, lambda self, v: setattr(self, 'reg_feat', v))})
    return model


def _members(n, n_layers=2):
    make_golden.import_reference()
    from models.caption import Transformer
    from models.caption.detector import build_detector
    out = []
    for i in range(n):
        cfg = make_golden._cfg(**{'model.cap_generator.n_layers': n_layers, 'model.decoder.decoder_name': 'parallel'})
        model = Transformer(build_detector(cfg), cfg)
        make_golden._fill()(model, 'e%d.' % i)
        model.eval()
        model.cached_features = True
        out.append(_alias_for_reference_ensemble(model))
    return out, cfg


def make_g16():
    make_golden.import_reference()
    from models.caption.ensemble import Ensemble
    B, Ng, Nr = 3, 16, 150
    gen = torch.Generator().manual_seed(16)
    # features on a 1/16 grid, stored as int8 codes (feature = code / 16): the file stays far below the size limit
    gri_q = (torch.randn(B, Ng, 1024, generator=gen) * 16).round().clamp(-127, 127).to(torch.int8)
    reg_q = (torch.randn(B, Nr, 512, generator=gen) * 16).round().clamp(-127, 127).to(torch.int8)
    gri_q[1, Ng - 4:] = 0
    gri, reg = gri_q.float() / 16, reg_q.float() / 16
    gri_mask = torch.zeros(B, 1, 1, Ng, dtype=torch.bool)
    gri_mask[1, ..., Ng - 4:] = True
    reg_mask = torch.zeros(B, 1, 1, Nr, dtype=torch.bool)
    out = {'gri_feat_q16': gri_q.numpy(), 'gri_mask': gri_mask.numpy(), 'reg_feat_q16': reg_q.numpy(), 'reg_mask': reg_mask.numpy()}
    members, cfg = _members(3)
    for K in (2, 3):
        ens = Ensemble(members[:K], bos_idx=cfg.model.bos_idx, config=cfg)
        for beam, out_size in ((1, 1), (5, 1), (5, 5)):
            record = []
            orig = ens.select

            def select(t, cand, beam_size, _orig=orig, _rec=record, **kw):
                flat = cand.reshape(cand.shape[0], -1)
                _rec.append(torch.sort(flat, -1, descending=True)[0][:, :beam_size + 1].clone())
                return _orig(t, cand, beam_size, **kw)

            ens.select = select
            with torch.no_grad():
                # the reference class reads the region features of `samples` under 'det_feat' too
                vis = {'gri_feat': gri.clone(), 'gri_mask': gri_mask.clone(), 'det_feat': reg.clone(), 'reg_mask': reg_mask.clone()}
                toks, lps = ens(vis, seq=None, use_beam_search=True, max_len=20, eos_idx=3, beam_size=beam, out_size=out_size)
            ens.select = orig
            top = torch.stack(record, 1)  # [B, steps, beam + 1]
            tag = 'k%d_b%d_o%d' % (K, beam, out_size)
            out.update({tag + '_tokens': toks.numpy(), tag + '_logprobs': lps.numpy(), tag + '_top': top.numpy()})
            margin = (top[..., :-1] - top[..., 1:]).abs().amin().item()
            print('g16', tag, toks.reshape(B, -1)[:, :8].tolist(), 'min margin between consecutive candidates', margin)
    np.savez_compressed(os.path.join(HERE, 'ensemble_g16.npz'), **out)


if __name__ == '__main__':
    torch.set_num_threads(8)
    make_g16()
