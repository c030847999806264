"""The float64 restatement of the Whisper ASR metric (include/tdvc.h, "The Whisper ASR metric") in plain torch and numpy: features,
encoder, decoder step with a cache, the greedy loop, WER / CER. It is pinned to HF transformers' own float64 output by
tests/golden/whisper_small.npz, whisper_small_audio.npz and whisper_heads.npz (tools/make_golden_whisper.py) and is what the GPU tests
measure against at other shapes. Nothing here imports transformers."""
import json
import math
import os

import numpy as np
import torch

HOP, NFFT, BINS, SR = 160, 400, 201, 16000


# ---------------------------------------------------------------------------------------------------------------- features
def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)), 200.0 * m / 3.0)


def mel_filters(n_mels=80):
    """[201][n_mels] float64: triangles on the Slaney mel scale from 0 to 8000 Hz, each divided by half its width in Hz."""
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(8000.0), n_mels + 2))
    bins = np.linspace(0.0, SR // 2, BINS)
    width = np.diff(edges)
    slopes = edges[None, :] - bins[:, None]
    fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / width[:-1], slopes[:, 2:] / width[1:]))
    return fb * (2.0 / (edges[2:] - edges[:-2]))[None, :]


def log_mel(x, lengths=None, n_samples=480000, n_mels=80):
    """x [B][L] -> float64 [B][n_mels][n_samples / 160]; samples at and past lengths[b] count as zeros (and are not read)."""
    x = np.asarray(x)
    B = x.shape[0]
    fb = mel_filters(n_mels)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)
    out = np.empty((B, n_mels, n_samples // HOP))
    for b in range(B):
        n = min(x.shape[1], n_samples, x.shape[1] if lengths is None else max(int(lengths[b]), 0))
        row = np.zeros(n_samples)
        row[:n] = x[b, :n].astype(np.float64)
        padded = np.pad(row, NFFT // 2, mode='reflect')
        frames = np.lib.stride_tricks.sliding_window_view(padded, NFFT)[::HOP][:n_samples // HOP]
        power = np.abs(np.fft.rfft(frames * win, axis=1)) ** 2
        v = np.log10(np.maximum(power @ fb, 1e-10)).T
        out[b] = (np.maximum(v, v.max() - 8.0) + 4.0) / 4.0
    return out


# ------------------------------------------------------------------------------------------------------------------ network
def load(z, prefix=''):
    """(cfg dict, state dict in float64) of the fixture z under `prefix` ('' | 'w16/' | 'w64/')."""
    cfg = json.loads(str(z[prefix + 'cfg']))
    sd = {k[len(prefix) + 3:]: torch.from_numpy(z[k].astype(np.float64)) for k in z.files if k.startswith(prefix + 'sd/')}
    return cfg, sd


def expected_shapes(cfg, proj_out=False):
    d, v = cfg['d_model'], cfg['vocab_size']
    out = {'model.encoder.conv1.weight': (d, cfg['num_mel_bins'], 3), 'model.encoder.conv1.bias': (d,), 'model.encoder.conv2.weight': (d, d, 3),
           'model.encoder.conv2.bias': (d,), 'model.encoder.embed_positions.weight': (cfg['max_source_positions'], d),
           'model.decoder.embed_tokens.weight': (v, d), 'model.decoder.embed_positions.weight': (cfg['max_target_positions'], d)}

    def attn(p):
        for n in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            out[f'{p}.{n}.weight'] = (d, d)
            if n != 'k_proj':
                out[f'{p}.{n}.bias'] = (d,)

    def norm(p):
        out[p + '.weight'] = out[p + '.bias'] = (d,)
    for half, nl, ffn in (('encoder', cfg['encoder_layers'], cfg['encoder_ffn_dim']), ('decoder', cfg['decoder_layers'], cfg['decoder_ffn_dim'])):
        for i in range(nl):
            p = f'model.{half}.layers.{i}'
            attn(p + '.self_attn'), norm(p + '.self_attn_layer_norm'), norm(p + '.final_layer_norm')
            if half == 'decoder':
                attn(p + '.encoder_attn'), norm(p + '.encoder_attn_layer_norm')
            out[p + '.fc1.weight'], out[p + '.fc1.bias'], out[p + '.fc2.weight'], out[p + '.fc2.bias'] = (ffn, d), (ffn,), (d, ffn), (d,)
        norm(f'model.{half}.layer_norm')
    if proj_out:
        out['proj_out.weight'] = (v, d)
    return out


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, sd, p):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * sd[p + '.weight'] + sd[p + '.bias']


def linear(x, sd, p):
    y = x @ sd[p + '.weight'].t()
    return y + sd[p + '.bias'] if p + '.bias' in sd else y


def _heads(x, h):
    return x.reshape(*x.shape[:-1], h, x.shape[-1] // h).transpose(-2, -3)          # [..., T, d] -> [..., h, T, d / h]


def attend(q, k, v, h):
    """q [.., Tq, d] (already scaled), k, v [.., Tk, d] -> [.., Tq, d], a plain softmax over all Tk keys."""
    qh, kh, vh = _heads(q, h), _heads(k, h), _heads(v, h)
    o = torch.softmax(qh @ kh.transpose(-1, -2), dim=-1) @ vh
    return o.transpose(-2, -3).reshape(q.shape)


def mlp(x, sd, p):
    return x + linear(gelu(linear(layer_norm(x, sd, p + '.final_layer_norm'), sd, p + '.fc1')), sd, p + '.fc2')


def encode(sd, cfg, feats):
    """feats [B][n_mels][frames] -> [B][frames / 2][d]."""
    x = torch.as_tensor(feats, dtype=sd['model.encoder.conv1.weight'].dtype)
    F = torch.nn.functional
    x = gelu(F.conv1d(x, sd['model.encoder.conv1.weight'], sd['model.encoder.conv1.bias'], padding=1))
    x = gelu(F.conv1d(x, sd['model.encoder.conv2.weight'], sd['model.encoder.conv2.bias'], stride=2, padding=1)).transpose(1, 2)
    x = x + sd['model.encoder.embed_positions.weight'][:x.shape[1]]
    h, d = cfg['encoder_attention_heads'], cfg['d_model']
    for i in range(cfg['encoder_layers']):
        p = f'model.encoder.layers.{i}'
        y = layer_norm(x, sd, p + '.self_attn_layer_norm')
        a = attend(linear(y, sd, p + '.self_attn.q_proj') * (d // h) ** -0.5, linear(y, sd, p + '.self_attn.k_proj'), linear(y, sd, p + '.self_attn.v_proj'), h)
        x = mlp(x + linear(a, sd, p + '.self_attn.out_proj'), sd, p)
    return layer_norm(x, sd, 'model.encoder.layer_norm')


class Decoder:
    """The step with its cache for rows enc [B][T_enc][d]: step(tokens [B], p) -> logits [B][vocab]."""

    def __init__(self, sd, cfg, enc):
        self.sd, self.cfg, self.h, self.scale = sd, cfg, cfg['decoder_attention_heads'], (cfg['d_model'] // cfg['decoder_attention_heads']) ** -0.5
        self.cross = [(linear(enc, sd, f'model.decoder.layers.{i}.encoder_attn.k_proj'), linear(enc, sd, f'model.decoder.layers.{i}.encoder_attn.v_proj'))
                      for i in range(cfg['decoder_layers'])]
        self.k = [[] for _ in self.cross]
        self.v = [[] for _ in self.cross]

    def step(self, tokens, p):
        sd = self.sd
        x = (sd['model.decoder.embed_tokens.weight'][torch.as_tensor(tokens, dtype=torch.long)] + sd['model.decoder.embed_positions.weight'][p])[:, None]
        for i, (ck, cv) in enumerate(self.cross):
            q = f'model.decoder.layers.{i}'
            y = layer_norm(x, sd, q + '.self_attn_layer_norm')
            self.k[i].append(linear(y, sd, q + '.self_attn.k_proj'))
            self.v[i].append(linear(y, sd, q + '.self_attn.v_proj'))
            assert len(self.k[i]) == p + 1
            a = attend(linear(y, sd, q + '.self_attn.q_proj') * self.scale, torch.cat(self.k[i], 1), torch.cat(self.v[i], 1), self.h)
            x = x + linear(a, sd, q + '.self_attn.out_proj')
            y = layer_norm(x, sd, q + '.encoder_attn_layer_norm')
            x = x + linear(attend(linear(y, sd, q + '.encoder_attn.q_proj') * self.scale, ck, cv, self.h), sd, q + '.encoder_attn.out_proj')
            x = mlp(x, sd, q)
        return layer_norm(x[:, 0], sd, 'model.decoder.layer_norm') @ sd['model.decoder.embed_tokens.weight'].t()


def step_logits(sd, cfg, enc, ids):
    """Teacher-forced logits [B][L][vocab] at every position of ids [B][L]."""
    dec = Decoder(sd, cfg, enc)
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.long)
    return torch.stack([dec.step(ids[:, p], p) for p in range(ids.shape[1])], 1)


def greedy(sd, cfg, enc, prompt, max_new_tokens, suppress=(), begin_suppress=(), eos=0, pad=0):
    """(ids [B][P + max_new_tokens], n_tokens [B], margins [B][max_new_tokens]): the argmax with the lowest index on ties."""
    B, P = enc.shape[0], len(prompt)
    dec = Decoder(sd, cfg, enc)
    ids = np.full((B, P + max_new_tokens), pad, dtype=np.int32)
    ids[:, :P] = np.asarray(prompt)
    n_tokens, done, margins = np.full(B, P, dtype=np.int32), np.zeros(B, dtype=bool), np.full((B, max_new_tokens), np.nan)
    for p in range(P + max_new_tokens - 1):
        logits = dec.step(ids[:, p], p).clone()
        if p + 1 < P:
            continue
        logits[:, list(suppress)] = -math.inf
        if p + 1 == P:
            logits[:, list(begin_suppress)] = -math.inf
        for b in range(B):
            if done[b]:
                continue
            top = torch.topk(logits[b], 2).values
            margins[b, p + 1 - P] = float(top[0] - top[1])
            tok = int(torch.nonzero(logits[b] == top[0])[0])
            ids[b, p + 1], n_tokens[b], done[b] = tok, p + 2, tok == eos
    return ids, n_tokens, margins


# ---------------------------------------------------------------------------------------------------------------- WER / CER
def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def wer(predictions, references):
    return sum(edit_distance(r.split(), p.split()) for p, r in zip(predictions, references)) / sum(len(r.split()) for r in references)


def cer(predictions, references):
    return sum(edit_distance(list(r), list(p)) for p, r in zip(predictions, references)) / sum(len(r) for r in references)


# ------------------------------------------------------------------------------------------------------------------ pinning
def pin_against(golden):
    """How far this restatement is from the fixtures: relative to the largest magnitude, and the number of unequal ids."""
    z, a, hz = (np.load(os.path.join(golden, n)) for n in ('whisper_small.npz', 'whisper_small_audio.npz', 'whisper_heads.npz'))
    cfg, sd = load(z)
    rel = lambda got, want: float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(np.asarray(want)).max())
    feats = torch.from_numpy(a['features'].astype(np.float64))
    enc = encode(sd, cfg, feats)
    out = dict(mel_filters=rel(mel_filters(80), z['mel_filters']),
               features_abs=float(np.abs(log_mel(a['input'], a['lengths'], n_samples=a['input'].shape[1]) - a['features'].astype(np.float64)).max()),
               enc=rel(enc, z['enc']), logits=rel(step_logits(sd, cfg, torch.from_numpy(z['enc']), z['ids']), z['logits']))
    ids, n_tokens, margins = greedy(sd, cfg, torch.from_numpy(z['enc']), z['prompt'], z['ids'].shape[1] - len(z['prompt']), z['suppress'], z['begin_suppress'],
                                    int(z['eos']), int(z['pad']))
    out['unequal_ids'] = int((ids != z['ids']).sum()) + int((n_tokens != z['n_tokens']).sum())
    out['margins'] = float(np.nanmax(np.abs(margins - z['margins'])))
    for tag in ('w16/', 'w64/'):
        c, s = load(hz, tag)
        e = encode(s, c, feats[1:2])
        out[tag + 'enc'] = rel(e[0], hz[tag + 'enc'])
        out[tag + 'logits'] = rel(step_logits(s, c, torch.from_numpy(hz[tag + 'enc'])[None], hz[tag + 'ids'])[0], hz[tag + 'logits'])
    return out
