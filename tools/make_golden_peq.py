"""Writes tests/golden/peq.npz and tests/golden/peq.json: the fixture that pins tests/peq_ref.py (the float64 truth of the GPU
tests of tdvc_peq_sos / tdvc_sos_filter) to the reference's own `random_eq` + `eq_rms_signals`.

    python tools/make_golden_peq.py [path/to/reference]

Runs where the reference checkout and scipy are present (default /root/reference). util/contentvec/audio_utils.py and
audio_corruption.py are loaded by path; audio_utils imports parselmouth at module level (for the Praat step whose result
corrupt_audio discards), so an empty stub module stands under that name while they load. The two files hold data only.

`speech` (2 x 4000): per row, np.random is seeded, the reference's random_eq runs on the fp32 signal, and the same seed is replayed
to recover its draws in draw order (z, then G). Stored: the signal, G, z, the reference's sos (params2sos on those draws), its
float64 sosfilt output and the eq_rms_signals output. `sections`: three arbitrary stable sections that are no EQ bands (run on
speech row 0 with S = 1 and S = 3). `odd` and `long` keep a probe of their regenerated signals only.

Asserted here, recorded in peq.json, and checked again by tests/test_corrupt_cpu.py: the restatement reproduces the reference to
1e-13 relative on sos and on both outputs (relative to the row maximum); for every GPU case the restatement agrees with
scipy.signal.sosfilt to the same 1e-13; and the fp32 restatement misses the GPU bound by the recorded factor.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import scipy.signal as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import peq_ref as PR  # noqa: E402

SPEECH_SEEDS = (1234, 7)
SPEECH_SIGNAL_SEED = 2024
T = 4000


def load_reference(root):
    """(audio_corruption, eq_rms_signals) from the reference tree, by path."""
    sys.modules.setdefault('parselmouth', types.ModuleType('parselmouth'))
    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m
    cv = os.path.join(root, 'util', 'contentvec')
    sys.path.insert(0, root)
    util = importlib.import_module('util')       # the reference's util package: eq_rms_signals (util/__init__.py:58-62)
    sys.modules.setdefault('util.contentvec', types.ModuleType('util.contentvec'))
    au = load('util.contentvec.audio_utils', os.path.join(cv, 'audio_utils.py'))
    sys.modules['util.contentvec'].audio_utils = au      # audio_corruption imports it by its dotted name
    ac = load('util.contentvec.audio_corruption', os.path.join(cv, 'audio_corruption.py'))
    return au, ac, util.eq_rms_signals


def relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def main():
    au, ac, eq_rms_signals = load_reference(sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
    assert np.array_equal(ac.Fc, PR.FC) and (ac.Qmin, ac.Qmax) == (PR.QMIN, PR.QMAX)
    arrays, meta = {}, {}

    rng = np.random.default_rng(SPEECH_SIGNAL_SEED)
    x = np.stack([PR.make_signal(rng, T, PR.SR) for _ in SPEECH_SEEDS])
    G, Z, SOS, Y, YR = [], [], [], [], []
    for row, seed in zip(x.astype(np.float64), SPEECH_SEEDS):      # float64, as sf.read hands the signal to corrupt_audio
        np.random.seed(seed)
        y = ac.random_eq(row, PR.SR)                       # the reference's own call: draws z, then G
        np.random.seed(seed)
        z = np.random.uniform(0, 1, size=(10,))
        g = np.random.uniform(-12, 12, size=(10,))
        sos = au.params2sos(g, ac.Fc, ac.Qmin * (ac.Qmax / ac.Qmin) ** z, PR.SR)
        assert np.array_equal(sps.sosfilt(sos, row), y), 'the replayed draws do not reproduce random_eq'
        G.append(g); Z.append(z); SOS.append(sos); Y.append(y); YR.append(eq_rms_signals(y, row))
    G, Z, SOS, Y, YR = map(np.stack, (G, Z, SOS, Y, YR))
    h_sos, h_y = PR.random_eq(x, G, Z, match=False)
    h_yr = PR.match_rms(h_y, x)
    meta['speech'] = dict(seeds=list(SPEECH_SEEDS), signal_seed=SPEECH_SIGNAL_SEED,
                          helper_sos_rel=relmax(h_sos, SOS), helper_y_rel=max(relmax(a, b) for a, b in zip(h_y, Y)),
                          helper_y_rms_rel=max(relmax(a, b) for a, b in zip(h_yr, YR)))
    assert max(meta['speech'][k] for k in ('helper_sos_rel', 'helper_y_rel', 'helper_y_rms_rel')) <= 1e-13, meta['speech']
    arrays.update(speech_signal=x, speech_G=G, speech_z=Z, speech_sos=SOS, speech_y=Y, speech_y_rms=YR)

    # arbitrary stable sections (poles at radius 0.9 / 0.99 / 0.5, zeros anywhere): the section count is not hard-wired to 10
    sec = np.array([[0.5, -0.3, 0.2, 1.0, -2 * 0.9 * np.cos(0.3), 0.81],
                    [1.2, 0.7, -0.4, 1.0, -2 * 0.99 * np.cos(1.1), 0.9801],
                    [0.8, 0.0, 0.1, 1.0, -2 * 0.5 * np.cos(2.5), 0.25]])
    arrays.update(sections_sos=sec)
    meta['sections'] = dict(helper_y_rel=max(relmax(PR.sosfilt(sec[:n], x[0]), sps.sosfilt(sec[:n], x[0].astype(np.float64))) for n in (1, 3)))
    assert meta['sections']['helper_y_rel'] <= 1e-13, meta['sections']

    for name, B, TT, seed in (('odd', PR.ODD_B, PR.ODD_T, PR.ODD_SEED), ('long', 1, PR.LONG_T, PR.LONG_SEED)):
        r = np.random.default_rng(seed)
        sig = np.stack([PR.make_signal(r, TT, PR.SR) for _ in range(B)]).reshape(-1)
        probe = np.arange(0, sig.size, max(1, sig.size // 256))
        arrays.update({f'{name}_probe_idx': probe.astype(np.int32), f'{name}_probe_val': sig[probe]})

    out = os.path.join(ROOT, 'tests', 'golden')
    np.savez_compressed(os.path.join(out, 'peq.npz'), **arrays)
    with open(os.path.join(out, 'peq.json'), 'w') as f:      # the cases below read the fixture back through peq_ref
        json.dump({'sample_rate': PR.SR, 'cases': meta}, f, indent=1)
    PR.fixture.cache_clear()

    # every GPU case: restatement against the reference's params2sos + scipy's sosfilt, and how far an fp32 cascade misses the bound
    for name in PR.CASES:
        t = PR.truth(name)
        ref_sos = np.stack([au.params2sos(g, ac.Fc, q, PR.SR) for g, q in zip(t['G'].astype(np.float64), t['Q'].astype(np.float64))])
        ref_y = np.stack([sps.sosfilt(s, r) for s, r in zip(ref_sos, t['x'])])
        s = dict(B=int(t['x'].shape[0]), T=int(t['x'].shape[1]), helper_sos_rel=relmax(t['sos'], ref_sos),
                 helper_y_rel=max(relmax(a, b) if np.abs(b).max() > 0 else float(np.abs(a).max()) for a, b in zip(t['y'], ref_y)))
        assert s['helper_sos_rel'] <= 1e-13 and s['helper_y_rel'] <= 1e-13, (name, s)
        bd = PR.bound(t['y'])
        if bd.max() > 0:
            s['fp32_over_bound'] = float((np.abs(PR.fp32_run(name) - t['y']) / np.where(bd > 0, bd, 1)).max(-1).min())
            s['round_once_over_bound'] = float((np.abs(t['y'].astype(np.float32) - t['y']) / np.where(bd > 0, bd, 1)).max())
        if name in PR.SPEECH_LIKE:
            assert s['fp32_over_bound'] >= 50, (name, s)
        meta[name] = {**meta.get(name, {}), **s}
        print(name, json.dumps(meta[name]))
    # random_eq end to end: the draws rounded to fp32 (as tdvc_peq_sos takes them) against the reference's float64 draws
    t = PR.truth('speech')
    meta['speech']['fp32_draws_over_bound'] = float((np.abs(t['y_rms'] - YR) / PR.bound(YR)).max())
    print('speech: fp32-rounded draws move the result by', meta['speech']['fp32_draws_over_bound'], 'of the bound')
    with open(os.path.join(out, 'peq.json'), 'w') as f:
        json.dump({'sample_rate': PR.SR, 'cases': meta}, f, indent=1)
    size = {n: os.path.getsize(os.path.join(out, n)) for n in ('peq.npz', 'peq.json')}
    assert size['peq.npz'] <= os.path.getsize(os.path.join(out, 'yin.npz')), size
    print('wrote', size)


if __name__ == '__main__':
    main()
