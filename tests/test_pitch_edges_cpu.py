"""CPU: the edge-case fixture (tests/golden/yin_edges.npz + yin_edges.json, tools/make_golden_yin_edges.py) still pins
tests/yin_edges_ref.py to the reference's float64 results at every row of the table and still meets the conditions its generator
asserted; tdvc_yin_num_frames and tdvc_yin_soft_bwd_workspace at every row; and the table still reaches the paths it was drawn up
for, by the mirror of the host code's plan that yin_edges_ref keeps."""
import os

import numpy as np
import pytest
import torch

import yin_edges_ref as ER
import yin_ref as YR
from common import pkg

CASES = tuple(ER.CASES)


@pytest.mark.parametrize('name', CASES)
def test_fixture_pins_helper_to_reference(name):
    """Hard f0 exactly, soft f0, the sampled CMDF entries within 1e-12 and the sampled gradient entries within 1e-9 of the row's max
    |gradient| (zero rows exactly) against what the reference computed in float64; the generator's conditions, recomputed."""
    meta, g = ER.fixture()
    assert (meta['sample_rate'], meta['threshold']) == (ER.SR, ER.THR) and tuple(meta['cases']) == CASES
    t = ER.truth(name)
    s, st = t['meta'], t['settings']
    assert {k: s[k] for k in st} == st
    assert t['x'].dtype == torch.float32 and tuple(t['x'].shape) == (s['B'], s['T'])
    assert t['hard'].shape == (s['B'], s['n_frames']) == g[f'{name}_f0_hard'].shape and t['cmdf'].shape[-1] == s['n']
    assert torch.equal(t['hard'], torch.from_numpy(g[f'{name}_f0_hard']))
    assert float((t['soft'] - torch.from_numpy(g[f'{name}_f0_soft'])).abs().max()) <= 1e-9 * ER.SR
    idx, val = g[f'{name}_cmdf_idx'], g[f'{name}_cmdf_val']
    assert len(idx) == min(ER.N_SAMPLED, t['cmdf'].numel()) and len(np.unique(idx)) == len(idx)
    assert float(np.abs(t['cmdf'].reshape(-1).numpy()[idx] - val).max()) <= 1e-12
    # recorded by the generator, and recomputed
    assert s['helper_hard_equals_reference'] and s['helper_cmdf_max_abs_diff'] <= 1e-12
    assert s['tol'] == 4 * min(s['E_ref32'], s['E_plain32']) and s['tol'] > 0
    assert float((~t['ok']).double().mean()) == s['excused_frac'] <= 0.05
    assert float(t['thr_margin'].min()) == pytest.approx(s['min_margin'], rel=1e-9) and float(t['thr_margin'].min()) > 2 * s['tol']
    on, voiced = float(t['on'].double().mean()), float((t['hard'] > 0).double().mean())
    assert on == pytest.approx(s['on_frac']) and voiced == pytest.approx(s['voiced_frac'])
    assert torch.equal(t['on'], t['soft'] > 0)
    if name == 'one33':
        # one sample: frames 0 .. 2 hold it and are non-periodic, frames 3 and 4 are all zero (on for the soft track, index 0 for the hard one)
        assert voiced == 0.0 and t['on'].tolist() == [[False, False, False, True, True]] and float(t['x'][0, 0]) == pytest.approx(0.02)
    else:
        assert 0.1 <= on <= 0.9, on
        if s['n'] >= 4:
            assert voiced > 0
    if name in ER.FORWARD_ONLY:
        assert t['dx'] is None and 'tol_g' not in s
        return
    assert tuple(t['dx'].shape) == (s['B'], s['T']) and tuple(t['gy'].shape) == (s['B'], s['n_frames']) and bool(torch.isfinite(t['dx']).all())
    assert torch.equal(t['gy'], t['gy'].float().double())
    idx, val, row_max = g[f'{name}_grad_idx'], g[f'{name}_grad_val'], g[f'{name}_row_max']
    assert len(idx) == min(ER.N_SAMPLED, t['dx'].numel()) and len(np.unique(idx)) == len(idx)
    rows = idx // s['T']
    err = np.abs(t['dx'].reshape(-1).numpy()[idx] - val)
    live = row_max[rows] > 0
    assert not err[~live].any() and not val[~live].any()
    assert float((err[live] / row_max[rows][live]).max(initial=0.0)) <= 1e-9
    assert np.allclose(t['dx'].abs().amax(-1).numpy(), row_max, rtol=1e-9, atol=0)
    assert [int(i) for i in np.nonzero(row_max == 0)[0]] == s['zero_rows'] and len(s['zero_rows']) < s['B']
    assert s['helper_grad_vs_reference'] <= 1e-9 and s['helper_zero_rows_match']
    assert s['tol_g'] == 4 * min(s['Eg_ref32'], s['Eg_plain32']) and 0 < s['tol_g'] <= 1e-4
    if name == 'odd267':
        z = (t['gy'] == 0)
        assert 0.3 <= float(z.double().mean()) <= 0.7 and bool((t['on'] & z).any()) and bool((t['on'] & ~z).any())
    else:
        assert not bool((t['gy'] == 0).any())


def test_fixture_is_small():
    size = sum(os.path.getsize(os.path.join(ER.GOLDEN, n)) for n in ('yin_edges.npz', 'yin_edges.json'))
    assert size <= 300 * 1024, size


def test_num_frames_and_workspace_at_every_row():
    lib = pkg()._lib.lib()
    for name in CASES:
        s = ER.settings(name)
        nf = YR.num_frames(s['T'], s['tau_max'], s['stride'])
        assert lib.tdvc_yin_num_frames(s['T'], s['tau_max'], s['stride']) == nf == s['n_frames'], name
        assert lib.tdvc_yin_soft_bwd_workspace(s['B'], s['T'], s['tau_max'], s['stride']) == s['B'] * nf * s['L'] * 4, name


# what each row was drawn up for: name -> the plan values the issue's table names (yin_edges_ref.plan)
REACHES = {
    'odd267': dict(NC=3, NCm=7, rounds=4),
    'cap1024': dict(NG=256, NC=1, NCm=1, rounds=2),
    'odd1023': dict(NG=256, NC=1),
    'nc4_255': dict(NG=64, NC=4),
    'nc2_401': dict(NC=2, NCm=5),
    'gap64': dict(NC=16, NCm=8, mslice=8),
    'dense21': dict(NG=6, NC=42),
    'n2_133': dict(NC=7),
    'tiny7': dict(NG=2, NC=128),
    'tiny5': dict(L=10),
    'tiny3': dict(L=6, NG=1, NC=256),
}


def test_table_reaches_the_edges_it_lists():
    S = {n: ER.settings(n) for n in CASES}
    P = {n: ER.plan(S[n]['tau_max']) for n in CASES}
    for name, want in REACHES.items():
        assert {k: P[name][k] for k in want} == want, (name, P[name])
    for name in CASES:
        p, s = P[name], S[name]
        assert p['NG'] * p['NC'] <= 256 and p['NCm'] * p['Lp'] <= 4096 and p['NCm'] * p['mslice'] >= p['M4'] and s['tau_max'] <= 1024 and s['n'] >= 2
    odd = [n for n in CASES if S[n]['L'] % 4 == 2]
    assert {'odd267', 'odd1023', 'nc4_255', 'nc2_401', 'dense21', 'n2_133', 'short101', 'tiny7', 'tiny5', 'tiny3', 'one33'} == set(odd)
    assert all(P[n]['Lp'] == S[n]['L'] + 2 for n in odd) and any(n in ER.BACKWARD_CASES and S[n]['tau_max'] >= 1023 for n in odd)
    assert S['cap1024']['n'] == 1023 and S['cap1024']['tau_max'] == 1024 and S['odd1023']['tau_max'] == 1023
    assert S['odd1023']['stride'] < S['odd1023']['L']
    assert {P[n]['NC'] for n in CASES} >= {1, 2, 3, 4} and any(P[n]['NC'] > 4 for n in ER.BACKWARD_CASES)
    assert sum(P[n]['NG'] < 64 for n in ER.BACKWARD_CASES) >= 3
    assert S['n2_133']['n'] == 2
    assert all(S[n]['stride'] > S[n]['L'] for n in ('gap64',)) and S['dense21']['stride'] == S['tiny5']['stride'] == 1
    assert S['short101']['T'] < S['short101']['L'] and S['short101']['B'] == 3 and S['one33']['T'] == 1
    assert set(ER.FORWARD_ONLY) == {'tiny3', 'one33'}
