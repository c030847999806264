"""Writes tests/golden/whisper_small.npz, whisper_small_audio.npz and whisper_heads.npz from HF transformers' own
WhisperForConditionalGeneration and WhisperFeatureExtractor on the CPU: the fixtures that pin td-vc-gan_amd/whisper.py's definition
(and tests/whisper_ref.py) to the real implementation. Run by hand where `transformers` is importable, never by a test:

    python tools/make_golden_whisper.py

No checkpoint is involved: the weights are seeded. Configuration `small`: vocab 203, d_model 64, 2 + 2 layers, 2 heads (head width
32), FFN 128, 80 mel bands, max_source_positions 100 (a 2 s chunk: 200 frames), max_target_positions 32. Weights are drawn with std
3 / sqrt(fan_in), biases with std 0.3, LayerNorm weights 1 + 0.3 n (with HF's default init the greedy sequence is one repeated
token), embed_positions of both halves included (they are read from the state dict), all rounded to float16-representable values and
stored as float16. Three input rows (noise, a tone, a chirp plus noise, 20000 / 32000 / 27000 samples, float16-representable):
  whisper_small_audio.npz   input [3][32000] fp16, lengths, features [3][80][200] fp32: WhisperFeatureExtractor's numpy path
                            (_np_extract_fbank_features on the zero-padded rows), float32 as it returns them
  whisper_small.npz         sd/<key> fp16, cfg (JSON), mel_filters [201][80] float64, and HF's float64 evaluation on those features:
                            enc [3][100][64], ids [3][32] (4 prompt tokens + 28 greedy tokens from a plain argmax loop with
                            suppress = [5, 7, 11, 150] and begin_suppress = [eos, 20]; pad after eos), n_tokens, logits [3][32][203]
                            teacher-forced on those ids at every position, margins [3][28] (top-1 minus top-2 of the suppressed
                            logits at every generated step; nan after eos)
  whisper_heads.npz         two tiny configurations (1 + 1 layers, FFN 64, vocab 51) with head widths 16 (4 heads) and 64 (1 head):
                            w16/sd/<key>, w16/cfg, w16/ids [1][8], w16/enc, w16/logits on row 1's features; the same under w64/
The tool asserts that its loop equals model.generate(do_sample=False, num_beams=1) with the same suppression, that every margin is at
least 1e-3, and that one row stops at eos before the cap while another reaches the cap; it searches seeds until all three hold.
whisper_small_pinning.json records the versions, the seed and how far tests/whisper_ref.py is from what was stored."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SOT, LANG, TASK, NOTS, EOS, PAD = 196, 197, 198, 199, 200, 201
PROMPT = [SOT, LANG, TASK, NOTS]
SUPPRESS, BEGIN = [5, 7, 11, 150], [EOS, 20]
NEW = 28
SMALL = dict(vocab_size=203, num_mel_bins=80, d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
             encoder_ffn_dim=128, decoder_ffn_dim=128, max_source_positions=100, max_target_positions=32, activation_function='gelu',
             scale_embedding=False, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0,
             pad_token_id=PAD, bos_token_id=EOS, eos_token_id=EOS, decoder_start_token_id=SOT)
TINY = dict(SMALL, vocab_size=51, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=64, decoder_ffn_dim=64, pad_token_id=50, bos_token_id=49,
            eos_token_id=49, decoder_start_token_id=48)


def build(cfg, seed):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    model = WhisperForConditionalGeneration(WhisperConfig(**cfg)).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            n = torch.randn(p.shape, generator=g)
            if 'layer_norm' in name and name.endswith('weight'):
                v = 1.0 + 0.3 * n
            elif p.dim() == 1:
                v = 0.3 * n
            else:
                v = n * 3.0 / float(p.shape[1:].numel()) ** 0.5
            p.copy_(v.half().float())
    model.tie_weights()
    assert model.proj_out.weight.data_ptr() == model.model.decoder.embed_tokens.weight.data_ptr()
    return model.double()


def signals():
    g = np.random.default_rng(20261021)
    n, sr = 32000, 16000.0
    t = np.arange(n) / sr
    rows = [0.05 * g.standard_normal(n), 0.3 * np.sin(2 * np.pi * 440.0 * t),
            0.2 * np.sin(2 * np.pi * (200.0 * t + 900.0 * t * t)) + 0.02 * g.standard_normal(n)]
    lengths = np.array([20000, 32000, 27000], dtype=np.int32)
    x = np.stack(rows).astype(np.float16)
    for i, ln in enumerate(lengths):
        x[i, ln:] = 0
    return x, lengths


def features(x):
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=80, sampling_rate=16000, hop_length=160, chunk_length=2, n_fft=400)
    assert fe.n_samples == x.shape[1] and fe.nb_max_frames == 200
    f = fe._np_extract_fbank_features(x.astype(np.float32), 'cpu')
    assert f.dtype == np.float32 and f.shape == (x.shape[0], 80, 200)          # HF rounds the log-mel values to float32 before the clamp
    return f, np.asarray(fe.mel_filters, dtype=np.float64)


def masked(logits, first):
    s = logits.clone()
    s[SUPPRESS] = -float('inf')
    if first:
        s[BEGIN] = -float('inf')
    return s


def greedy(model, feat):
    """ids [P + NEW], n_tokens, margins [NEW]: a plain argmax loop over the decoder with HF's own cache."""
    with torch.no_grad():
        enc = model.model.encoder(feat[None]).last_hidden_state
        ids, margins, past, done = list(PROMPT), [], None, False
        inp = torch.tensor([PROMPT])
        n_tokens = len(PROMPT)
        for step in range(NEW):
            out = model(decoder_input_ids=inp, encoder_outputs=(enc,), past_key_values=past, use_cache=True)
            past = out.past_key_values
            if done:
                ids.append(PAD)
                margins.append(float('nan'))
            else:
                s = masked(out.logits[0, -1], step == 0)
                top = torch.topk(s, 2).values
                margins.append(float(top[0] - top[1]))
                tok = int(torch.argmax(s))
                ids.append(tok)
                n_tokens += 1
                done = tok == EOS
            inp = torch.tensor([[ids[-1]]])
    return enc[0], ids, n_tokens, margins


def hf_generate(model, feat):
    from transformers import GenerationConfig
    model.generation_config = GenerationConfig(eos_token_id=EOS, pad_token_id=PAD, decoder_start_token_id=SOT, bos_token_id=EOS)
    with torch.no_grad():
        out = model.generate(input_features=feat[None], decoder_input_ids=torch.tensor([PROMPT]), do_sample=False, num_beams=1, max_new_tokens=NEW,
                             suppress_tokens=SUPPRESS, begin_suppress_tokens=BEGIN, return_timestamps=False)
    out = out[0].tolist() if torch.is_tensor(out) else out['sequences'][0].tolist()
    return out


def teacher(model, feat, ids):
    with torch.no_grad():
        return model(input_features=feat[None], decoder_input_ids=torch.tensor([ids])).logits[0]


def main():
    import transformers
    x, lengths = signals()
    feats32, mel = features(x)
    feats = torch.from_numpy(feats32).double()
    for seed in range(1, 400):
        model = build(SMALL, seed)
        runs = [greedy(model, feats[i]) for i in range(3)]
        stopped = [r[2] < len(PROMPT) + NEW for r in runs]
        mins = min(m for r in runs for m in r[3] if m == m)
        varied = min(len(set(r[1][len(PROMPT):r[2]])) for r in runs)
        print(f'seed {seed}: n_tokens {[r[2] for r in runs]} smallest margin {mins:.3e} distinct tokens {varied}')
        if any(stopped) and not all(stopped) and mins >= 1e-3 and varied >= 3:
            break
    else:
        raise SystemExit('no seed met the conditions')
    for i, r in enumerate(runs):
        hf = hf_generate(model, feats[i])
        new = r[1][len(PROMPT):r[2]]                                            # Whisper's generate returns the new tokens: no prompt, no final eos
        if hf[:len(PROMPT)] == PROMPT:
            hf = hf[len(PROMPT):]
        assert hf == (new[:-1] if new[-1] == EOS else new) or hf == new, (i, hf, r[1])
    ids = np.array([r[1] for r in runs], dtype=np.int32)
    logits = torch.stack([teacher(model, feats[i], runs[i][1]) for i in range(3)])
    assert logits.dtype == torch.float64 and tuple(logits.shape) == (3, len(PROMPT) + NEW, 203)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert all(torch.equal(v.half().double(), v) for v in sd.values())
    arrays = {'sd/' + k: v.half().numpy() for k, v in sd.items()}
    arrays.update(cfg=np.array(json.dumps(SMALL)), mel_filters=mel, enc=torch.stack([r[0] for r in runs]).numpy(), ids=ids,
                  n_tokens=np.array([r[2] for r in runs], dtype=np.int32), logits=logits.numpy(), margins=np.array([r[3] for r in runs]),
                  prompt=np.array(PROMPT, dtype=np.int32), suppress=np.array(SUPPRESS, dtype=np.int32), begin_suppress=np.array(BEGIN, dtype=np.int32),
                  eos=np.array(EOS), pad=np.array(PAD))
    path = os.path.join(GOLDEN, 'whisper_small.npz')
    np.savez_compressed(path, **arrays)
    apath = os.path.join(GOLDEN, 'whisper_small_audio.npz')
    np.savez_compressed(apath, input=x, lengths=lengths, features=feats32)
    heads = {}
    for tag, nh in (('w16', 4), ('w64', 1)):
        cfg = dict(TINY, encoder_attention_heads=nh, decoder_attention_heads=nh)
        m = build(cfg, 1000 + nh)
        tids = [48] + [int(v) for v in np.random.default_rng(nh).integers(0, 48, 7)]
        with torch.no_grad():
            enc = m.model.encoder(feats[1][None]).last_hidden_state[0]
        heads.update({f'{tag}/sd/{k}': v.half().numpy() for k, v in m.state_dict().items()})
        heads.update({f'{tag}/cfg': np.array(json.dumps(cfg)), f'{tag}/ids': np.array([tids], dtype=np.int32), f'{tag}/enc': enc.numpy(),
                      f'{tag}/logits': teacher(m, feats[1], tids).numpy()})
    hpath = os.path.join(GOLDEN, 'whisper_heads.npz')
    np.savez_compressed(hpath, **heads)
    for p in (path, apath, hpath):
        print(f'{p}: {os.path.getsize(p)} bytes')
        assert os.path.getsize(p) < (1 << 20)
    # how far the float64 restatement is from what was just stored
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import whisper_ref as R
    pin = dict(transformers=transformers.__version__, torch=torch.__version__, numpy=np.__version__, seed=seed, restatement=R.pin_against(GOLDEN))
    json.dump({'whisper_small': pin}, open(os.path.join(GOLDEN, 'whisper_small_pinning.json'), 'w'), indent=1)
    print('pinned:', pin)


if __name__ == '__main__':
    main()
