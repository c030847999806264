"""Times the speaker-similarity evaluation on the GPU (td-vc-gan_amd/speaker.py; csrc/eval_speaker.hip), per call:

    voice_mel             the mel front end alone (one launch: padded-row index mapping, float64 DFT, 40 mel sums)
    lstm_fwd              the 3-layer recurrence alone on that mel and its window list (per layer: two packing launches, the input
                          projection as one GEMM, the recurrence with a workgroup per 16 windows)
    embed_utterance       waveform in, utterance embeddings out: mel, window list, recurrence, linear + ReLU + norms
    speaker_similarity    the scoring of a 16-speaker set (80 reference and 48 test embeddings) in stock torch ops

beside comparators measured in the same session:

    torch_lstm            the same network as torch.nn.LSTM(40, 256, 3) + Linear in stock torch on the same device, on the same
                          windows gathered into [P, 160, 40] (the gather is not timed)
    generator_forward     one infer.convert forward of the same audio (config/conv_enc-stage1.yaml, weights as initialised)

    python tools/bench_speaker.py [--iters 20] [--warmup 3] [--rounds 5] [--torch-iters 5] [--out profiles/speaker_bench.txt]

Shapes: 16 x 4.48 s (71680 samples, 5 windows per row, 80 windows) and 1 x 20 s (25 windows) at 16 kHz; the signals of
tools/bench_mcd.py. Device time from events around `iters` back-to-back calls after a warm-up, the implementations alternating in
rounds; the median round is reported with the spread. One JSON line per shape, microseconds per call, printed and written to --out.
rec_us_per_step is lstm_fwd / (3 x 160): the recurrent step of one layer with its share of the projection.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _timing import measure, parse_args, report  # noqa: E402


def main():
    a = parse_args('bench_speaker', iters=20, warmup=3, rounds=5, torch_iters=5, out=os.path.join(ROOT, 'profiles', 'speaker_bench.txt'))
    import speaker_ref as R
    import tdvc_amd as P
    from bench_mcd import voiced_signal
    dev = torch.device('cuda:0')
    S = P.speaker
    hp = P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml'))
    G = P.infer.build_generator(hp.model.generator, 16, dev)
    sd = R.state_dict(seed=3)
    enc = P.VoiceEncoder()
    enc.load_state_dict(sd)
    enc = enc.to(dev).eval()
    stock = R.net(sd, torch.float32).to(dev)
    te, tt, re_, rs = (torch.from_numpy(t).to(dev) for t in R.similarity_case())
    lines = []
    for name, B, T in (('16 x 4.48 s', 16, 71680), ('1 x 20 s', 1, 320000)):
        rng = np.random.default_rng(B)
        test = voiced_signal(rng, B, T).to(dev)
        mel = S.voice_mel(test)
        utt, part, counts = enc.embed_utterance(test, return_partials=True)
        P_max = part.shape[1]
        step = S.frame_step()
        slots = torch.tensor([(b, j * step) for b in range(B) for j in range(P_max)], dtype=torch.int32, device=dev)
        wins = torch.stack([mel[b, s:s + 160] for b, s in slots.tolist()]).contiguous()
        w = enc._weights()

        def torch_lstm():
            with torch.no_grad():
                return R.embed(stock, R.hidden(stock, wins))

        c_tgt = torch.zeros(B, 16, device=dev); c_tgt[:, 3] = 1.0
        f0_conv = P.track_f0(test)
        noise = (torch.randn(B, 1, T, device=dev), torch.randn(B, 1, T, device=dev))
        phi0 = torch.tensor([0.5], device=dev)
        fns = {'voice_mel': (lambda: S.voice_mel(test), a.iters),
               'lstm_fwd': (lambda: S.lstm_fwd(mel, slots, w), a.iters),
               'embed_utterance': (lambda: enc.embed_utterance(test), a.iters),
               'speaker_similarity': (lambda: S.speaker_similarity(te, tt, re_, rs, 16), a.iters),
               'torch_lstm': (torch_lstm, a.torch_iters),
               'generator_forward': (lambda: P.infer.convert(G, test, c_tgt, f0_conv, noise=noise, start_phase=phi0), max(1, a.iters // 4))}
        try:
            gap = float((torch_lstm() - part.reshape(-1, 256)).abs().max())
        except RuntimeError as e:                                              # a build of torch without an LSTM on the device
            print(f'torch_lstm left out: {str(e)[:120]}', flush=True)
            del fns['torch_lstm']
            gap = None
        med, mm = measure(fns, a.warmup, a.rounds)
        out = {'shape': name, 'B': B, 'mel_frames': mel.shape[1], 'windows': int(counts.sum()), 'max_gap_to_torch_lstm': gap and float(f'{gap:.2e}'),
               **report(med, mm, 1)}
        out['rec_us_per_step'] = round(med['lstm_fwd'] / (3 * 160), 2)
        if 'torch_lstm' in med:
            out['torch_lstm_over_lstm_fwd'] = round(med['torch_lstm'] / med['lstm_fwd'], 2)
        out['embed_utterance_over_generator_forward'] = round(med['embed_utterance'] / med['generator_forward'], 3)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/bench_speaker.py on one MI355X (defaults: {a.iters} calls per timing, warm-up {a.warmup}, {a.rounds} rounds alternating the\n'
                f'# implementations, median and [min, max] in microseconds per call; torch_lstm {a.torch_iters} calls per round), 16 kHz.\n'
                '# The names are explained at the top of the tool.\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
