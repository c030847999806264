"""CPU: the train-step replay sequence (step_replay_cases.py) and its float64 fixtures (oracle/make_golden_replay.py).

What the GPU test (test_step_replay_gpu.py) can conclude from the fixtures rests on three things checked here without a GPU:
the input sets really differ where a stale value would otherwise go unnoticed, the fixtures really tell a stale batch from a
fresh one at the bar the GPU test uses, and the fixtures belong to this sequence (one oracle iteration reproduces them).
"""
import json

import pytest
import torch

import step_replay_cases as RC


def _gold(case):
    return json.load(open(RC.fixture_paths(case)[0]))


def test_sequence_shape():
    """Two warm-up iterations on input set 0, then three replays on three further sets; B = 3, T = 8960."""
    assert RC.SCHEDULE == (0, 0, 1, 2, 3) and RC.REPLAYED == (2, 3, 4)
    assert {c.name for c in RC.CASES} == {'stage2_2', 'stage1_switches', 'stage2_2_frozen_encoder', 'stage2_2_f0_yin'}
    assert {c.name for c in RC.FIXTURE_CASES} == {'stage2_2', 'stage1_switches'}
    for c in RC.CASES:
        assert (c.B, c.T) == (3, 8960) and len(c.inputs) > max(RC.SCHEDULE) + 1
        seeds = [s_ for s in c.inputs for s_ in (s.ix_seed, s.iy_seed)]
        assert len(set(seeds)) == len(seeds) and len({s.batch_seed for s in c.inputs}) == len(c.inputs)
    tr = RC.train_dict(RC.BY_NAME['stage1_switches'])
    assert (tr['lambda_latcls'], tr['grad_max_norm_D'], tr['grad_max_norm_G'], tr['jitter_amp']) == (1.0, 0.05, 0.5, 37)
    assert tr['lambda_idt'] > 0 and tr['lambda_f0'] == 0           # the jittered target enters the identity terms
    tr = RC.train_dict(RC.BY_NAME['stage2_2'])
    assert tr['lambda_rec'] > 0 and tr['lambda_f0'] == 0 and not tr['jitter_amp']
    assert RC.train_dict(RC.BY_NAME['stage2_2_f0_yin'])['lambda_f0'] == 1000.0
    assert RC.train_dict(RC.BY_NAME['stage2_2_frozen_encoder'])['freeze_subnets'] == ['encoder']


@pytest.mark.parametrize('case', RC.CASES, ids=lambda c: c.name)
def test_seed_conditions(case):
    """A stale label, conditioning vector, jitter shift or index table must change what the step computes: every set converts
    at least one sample to another speaker, consecutive sets have other source labels, consecutive jitter vectors differ in
    every element and hold both signs, and every refreshed tensor differs from its predecessor."""
    sets = [RC.input_set(case, k) for k in range(len(case.inputs))]
    for k, (bt, ix, iy) in enumerate(sets):
        assert (bt['label_tgt'] != bt['label_src']).any(), (k, bt['label_src'], bt['label_tgt'])
        assert torch.equal(bt['c_src'].argmax(1), bt['label_src']) and torch.equal(bt['c_tgt'].argmax(1), bt['label_tgt'])
        assert ix.dtype == torch.int64 and tuple(ix.shape) == (case.B, case.T // 320, 100) and not torch.equal(ix, iy)
        if 'jitter' in bt:
            j = bt['jitter']
            assert j.dtype == torch.int64 and tuple(j.shape) == (case.B,) and (j > 0).any() and (j < 0).any(), (k, j)
            assert int(j.abs().max()) <= RC.train_dict(case)['jitter_amp']
        if k:
            pb, pix, piy = sets[k - 1]
            assert tuple(bt['label_src'].tolist()) != tuple(pb['label_src'].tolist()), k
            assert set(bt) == set(pb)
            for key in bt:
                assert not torch.equal(bt[key], pb[key]), (k, key)
            assert not torch.equal(ix, pix) and not torch.equal(iy, piy)
            if 'jitter' in bt:
                assert (bt['jitter'] != pb['jitter']).all(), (k, bt['jitter'], pb['jitter'])
    assert ('jitter' in sets[0][0]) == (case.name == 'stage1_switches')
    assert ('f0_conv' in sets[0][0]) == (case.name == 'stage2_2_f0_yin')
    # the stale variants are set 0's tensors
    sb, six, _ = RC.input_set(case, 2, stale_batch=True)
    assert torch.equal(sb['signal_real'], sets[0][0]['signal_real']) and torch.equal(six, sets[2][1])
    fb, fix_, _ = RC.input_set(case, 2, stale_indices=True)
    assert torch.equal(fb['signal_real'], sets[2][0]['signal_real']) and torch.equal(fix_, sets[0][1])


@pytest.mark.parametrize('case', RC.FIXTURE_CASES, ids=lambda c: c.name)
def test_fixture_discriminates(case):
    """For every replayed iteration the stale-batch run differs from the fresh run by at least 10 x the 1e-3 bar on D_loss, on
    G_loss_adv_fake and on a *_feat scalar: a GPU step within 1e-3 of the fresh scalars cannot have used a stale batch. The
    stale-indices signal on G_loss_cont_emb is far below 1e-3 (only graph-against-eager can see it); it is printed and stored,
    because the GPU test's bar on that scalar is a tenth of it."""
    g = _gold(case)
    assert (g['case'], g['B'], g['T'], tuple(g['schedule'])) == (case.name, case.B, case.T, RC.SCHEDULE)
    assert g['inputs'] == [[s.batch_seed, s.ix_seed, s.iy_seed, s.jitter_seed] for s in case.inputs]
    assert g['train_overrides'] == case.train and g['dtype'] == 'float64'
    for run in ('fresh', 'stale_batch', 'stale_indices'):
        assert len(g[run]) == RC.ITERATIONS and all(set(r) == set(g['fresh'][0]) for r in g[run])
        assert g[run][:2] == g['fresh'][:2]            # set 0 either way
    assert set(g['next_fresh']) == set(g['fresh'][0])
    feat = [k for k in g['fresh'][0] if k.endswith('_feat')]
    assert feat
    for it in RC.REPLAYED:
        f, s = g['fresh'][it], g['stale_batch'][it]
        ch = {k: RC.rel_change(s[k], f[k]) for k in f}
        print(f'{case.name} it {it} stale batch: ' + ', '.join(f'{k} {v:.2e}' for k, v in ch.items()))
        assert ch['D_loss'] >= 10 * RC.TOL and ch['G_loss_adv_fake'] >= 10 * RC.TOL, (it, ch)
        assert max(ch[k] for k in feat) >= 10 * RC.TOL, (it, ch)
    sig = [RC.rel_change(g['stale_indices'][it]['G_loss_cont_emb'], g['fresh'][it]['G_loss_cont_emb']) for it in RC.REPLAYED]
    print(f'{case.name} stale indices, G_loss_cont_emb: {sig}; fp32 spread of the oracle: {max(g["fp32_spread"].values()):.2e}; '
          f'recipe {g["run_time_s"]} s')
    assert g['cont_emb_stale_indices_signal'] == min(sig) and min(sig) > 0
    # what the GPU bars assume: the oracle's own fp32 evaluation of the five iterations (rounding that four AdamW updates
    # have amplified: early Adam steps are ~lr * sign(g)) uses up at most a fifth of the 1e-3 bar, and the cont_emb cap
    # (signal / 10) is above the 1e-6 floor of the scalar comparison
    assert max(g['fp32_spread'].values()) < RC.TOL / 5
    assert min(sig) / 10 > 1e-6
    if case.train.get('grad_max_norm_D') is not None:      # every step really is clipped, on both optimizers
        assert len(g['grad_norms']) == RC.ITERATIONS
        for n in g['grad_norms']:
            assert n['D'] > 2 * case.train['grad_max_norm_D'] and n['G'] > 2 * case.train['grad_max_norm_G'], g['grad_norms']
    if 'jitter_amp' in case.train:                         # the jittered target enters a loss
        assert {'G_loss_idt_feat', 'G_loss_idt_spec', 'C_loss', 'G_loss_lat_cls'} <= set(g['fresh'][0])
    if case.name == 'stage2_2':
        assert {'G_loss_rec_feat', 'G_loss_rec_spec', 'G_loss_idt_feat'} <= set(g['fresh'][0])


@pytest.mark.parametrize('case', RC.FIXTURE_CASES, ids=lambda c: c.name)
def test_fixture_belongs_to_this_sequence(case):
    """One fp32 iteration of the oracle on input set 0 reproduces iteration 0 of the float64 fixture to 1e-5."""
    import importlib
    import os
    from oracle import step as OS
    synth = importlib.import_module('td-vc-gan_amd.synth')
    fill = lambda w: synth.fill_state_dict(json.load(open(os.path.join(RC.GOLDEN, f'shapes_{w}.json'))))
    cfg = OS.StepConfig.from_hparams(RC.train_dict(case))
    st = OS.TrainStep(fill('G'), fill('D'), cfg, fill('C') if cfg.lambda_latcls != 0 else None)
    got = st.run(*RC.input_set(case, 0))
    ref = _gold(case)['fresh'][0]
    assert set(got) == set(ref)
    errs = {k: RC.rel_change(got[k], v) for k, v in ref.items()}
    assert max(errs.values()) < 1e-5, errs
