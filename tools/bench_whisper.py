"""Times the Whisper ASR metric (td-vc-gan_amd/whisper.py) on one GPU at the whisper-medium shape with seeded weights, against the
same network in stock torch fp32 ops with a key/value cache on the same device, in the same process, rounds alternating:

    python tools/bench_whisper.py [--batches 1 16] [--rounds 3] [--small]      -> one JSON line per batch size

Per batch size B x 30 s: log_mel, encode, the cross k|v projection of all decoder layers, one decoder step launched eagerly and
replayed as a graph (position 32), the step's launch classes on their own (linear_step at N = 1024 from K = 1024 and from K = 4096,
N = 3072, N = 4096; attn_step over 33 cached keys and over the 1500 encoder keys; logits + pick), generate for 32 and 128 new tokens
(encoder output given), and `torch_*` the stock-torch restatement of the same quantities (greedy, argmax on the device, no host
synchronisation either). Times are medians over the rounds in microseconds, [min, max] beside them. For every step launch class
the bytes it must move (weights once, keys and values once) over its time is reported as GB/s, to be read beside the 6.29 TB/s
measured HBM copy rate of an MI355X. --small runs the fixture-sized network (a rehearsal of the tool, not a measurement)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 6290.0


def timed(fn, calls, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls


class TorchWhisper:
    """The same network in stock torch ops on the model's own parameters: encoder, cached decoder step, greedy loop."""

    def __init__(self, m):
        self.m, self.cfg = m, m.cfg
        self.sd = {k: v.detach() for k, v in m.state_dict().items()}

    def lin(self, x, p):
        return F.linear(x, self.sd[p + '.weight'], self.sd.get(p + '.bias'))

    def ln(self, x, p):
        return F.layer_norm(x, x.shape[-1:], self.sd[p + '.weight'], self.sd[p + '.bias'], 1e-5)

    def attn(self, q, k, v, h):
        B, Tq, d = q.shape
        sp = lambda t: t.view(B, t.shape[1], h, d // h).transpose(1, 2)
        return F.scaled_dot_product_attention(sp(q), sp(k), sp(v), scale=(d // h) ** -0.5).transpose(1, 2).reshape(B, Tq, d)

    def mlp(self, x, p):
        return x + self.lin(F.gelu(self.lin(self.ln(x, p + '.final_layer_norm'), p + '.fc1')), p + '.fc2')

    def encode(self, feats):
        sd, h = self.sd, self.cfg.encoder_attention_heads
        x = F.gelu(F.conv1d(feats, sd['model.encoder.conv1.weight'], sd['model.encoder.conv1.bias'], padding=1))
        x = F.gelu(F.conv1d(x, sd['model.encoder.conv2.weight'], sd['model.encoder.conv2.bias'], stride=2, padding=1)).transpose(1, 2)
        x = x + sd['model.encoder.embed_positions.weight']
        for i in range(self.cfg.encoder_layers):
            p = f'model.encoder.layers.{i}'
            y = self.ln(x, p + '.self_attn_layer_norm')
            a = self.attn(self.lin(y, p + '.self_attn.q_proj'), self.lin(y, p + '.self_attn.k_proj'), self.lin(y, p + '.self_attn.v_proj'), h)
            x = self.mlp(x + self.lin(a, p + '.self_attn.out_proj'), p)
        return self.ln(x, 'model.encoder.layer_norm')

    def cross(self, enc):
        return [(self.lin(enc, f'model.decoder.layers.{i}.encoder_attn.k_proj'), self.lin(enc, f'model.decoder.layers.{i}.encoder_attn.v_proj'))
                for i in range(self.cfg.decoder_layers)]

    def step(self, tok, p, cache, cross):
        """tok [B] at position p (host int) -> logits [B, vocab]; cache [layers][2][B][total][d] is filled at p."""
        sd, h = self.sd, self.cfg.decoder_attention_heads
        x = (sd['model.decoder.embed_tokens.weight'][tok] + sd['model.decoder.embed_positions.weight'][p])[:, None]
        for i, (ck, cv) in enumerate(cross):
            q = f'model.decoder.layers.{i}'
            y = self.ln(x, q + '.self_attn_layer_norm')
            cache[i, 0, :, p], cache[i, 1, :, p] = self.lin(y, q + '.self_attn.k_proj')[:, 0], self.lin(y, q + '.self_attn.v_proj')[:, 0]
            a = self.attn(self.lin(y, q + '.self_attn.q_proj'), cache[i, 0, :, :p + 1], cache[i, 1, :, :p + 1], h)
            x = x + self.lin(a, q + '.self_attn.out_proj')
            y = self.ln(x, q + '.encoder_attn_layer_norm')
            x = x + self.lin(self.attn(self.lin(y, q + '.encoder_attn.q_proj'), ck, cv, h), q + '.encoder_attn.out_proj')
            x = self.mlp(x, q)
        return F.linear(self.ln(x[:, 0], 'model.decoder.layer_norm'), sd['model.decoder.embed_tokens.weight'])

    def generate(self, enc, prompt, new, eos, pad):
        B, P, dev = enc.shape[0], len(prompt), enc.device
        total = P + new
        cross = self.cross(enc)
        cache = torch.empty(self.cfg.decoder_layers, 2, B, total, self.cfg.d_model, device=dev)
        ids = torch.full((B, total), pad, dtype=torch.long, device=dev)
        ids[:, :P] = torch.tensor(prompt, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        for p in range(total - 1):
            logits = self.step(ids[:, p], p, cache, cross)
            if p + 1 >= P:
                tok = torch.where(done, torch.full_like(ids[:, 0], pad), logits.argmax(-1))
                ids[:, p + 1] = tok
                done |= tok == eos
        return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    pkg = importlib.import_module('td-vc-gan_amd')
    w = pkg.whisper
    dev = torch.device('cuda:0')
    cfg = dict(w.MEDIUM)
    if args.small:
        cfg.update(vocab_size=203, d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=128,
                   decoder_ffn_dim=128, eos_token_id=200, pad_token_id=201)
    torch.manual_seed(20261021)
    m = w.Whisper(cfg)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0.0, 1.5 / float(p.shape[1:].numel()) ** 0.5)
            elif 'layer_norm' in name and name.endswith('weight'):
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            else:
                p.normal_(0.0, 0.1)
    m = m.to(dev)
    tw = TorchWhisper(m)
    c = m.cfg
    d, V, nl, ffn, T_enc, heads = c.d_model, c.vocab_size, c.decoder_layers, c.decoder_ffn_dim, c.max_source_positions, c.decoder_attention_heads
    prompt, eos, pad = [min(50258, V - 4), min(50259, V - 3), min(50359, V - 2), min(50363, V - 1)], c.eos_token_id, c.pad_token_id
    chunk = 2 * T_enc * 160 // 16000
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        x = (0.1 * torch.randn(B, chunk * 16000, generator=g)).to(dev)
        feats = w.whisper_log_mel(x, None, chunk)
        enc = m.encode(feats)
        gap = float((enc - tw.encode(feats)).abs().max())
        ids_h, _ = m.generate(None, prompt, 32, eos=eos, pad=pad, encoder_output=enc)
        ids_t = tw.generate(enc, prompt, 32, eos, pad)
        res = dict(shape=f'{B} x {chunk} s', B=B, encoder_gap_to_torch=gap, encoder_scale=float(enc.abs().max()),
                   ids_equal_torch_32=bool((ids_h.long() == ids_t).all()), first_difference=int((ids_h.long() != ids_t).any(0).float().argmax()))
        # the step's pieces at position 32: a state of 36 + 128 positions
        st = m._state(B, T_enc, 4 + 128, dev)
        st.ids.fill_(1), st.pos.fill_(32), st.mask.zero_()
        m._project_cross(st, enc)
        lay = m.model.decoder.layers[0]
        pk = m._pack(dev)
        pos32 = torch.full((1,), 32, dtype=torch.int32, device=dev)

        def reset_pos():
            st.pos.fill_(32)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            m._step(st, 4, eos, pad, None)
        wq, bq = pk['dec'][0]
        big = torch.empty(B, 3 * d, device=dev)
        cases = {
            'log_mel': (lambda: w.whisper_log_mel(x, None, chunk), 3, 0),
            'encode': (lambda: m.encode(feats), 2, 0),
            'cross_kv': (lambda: m._project_cross(st, enc), 2, 0),
            'step_eager': (lambda: (reset_pos(), m._step(st, 4, eos, pad, None)), 10, 0),
            'step_graph': (lambda: (reset_pos(), graph.replay()), 10, 0),
            'linear_n1024_k1024': (lambda: w.whisper_linear_step(st.att, lay.self_attn.out_proj.weight.detach(), lay.self_attn.out_proj.bias, residual=st.x, out=st.x), 50,
                                   4 * d * d),
            'linear_n3072_ln': (lambda: w.whisper_linear_step(st.x, wq, bq, norm=(lay.self_attn_layer_norm.weight, lay.self_attn_layer_norm.bias),
                                                              cache=(st.cache[0, 0], st.cache[0, 1], pos32, d), out=st.q), 50, 4 * 3 * d * d),
            'linear_n4096_ln_gelu': (lambda: w.whisper_linear_step(st.x, lay.fc1.weight.detach(), lay.fc1.bias, norm=(lay.final_layer_norm.weight, lay.final_layer_norm.bias),
                                                                   epilogue=w.EPI_GELU, out=st.ffn), 50, 4 * ffn * d),
            'linear_n1024_k4096': (lambda: w.whisper_linear_step(st.ffn, lay.fc2.weight.detach(), lay.fc2.bias, residual=st.x, out=st.x), 50, 4 * ffn * d),
            'attn_step_self_33': (lambda: w.whisper_attn_step(st.q, st.cache[0, 0], st.cache[0, 1], heads, pos=pos32, out=st.att), 50, 4 * 2 * B * 33 * d),
            'attn_step_cross': (lambda: w.whisper_attn_step(st.q, st.cross[0][:, :, :d], st.cross[0][:, :, d:], heads, out=st.att), 50, 4 * 2 * B * T_enc * d),
            'logits_pick': (lambda: (reset_pos(), w.whisper_logits(st.x, m.model.decoder.layer_norm.weight, m.model.decoder.layer_norm.bias,
                                                                  m.model.decoder.embed_tokens.weight.detach(), st.pos, 4, st.partials, mask=st.mask),
                                     w.whisper_pick(st.partials, V, st.ids, 4, eos, pad, st.pos, st.n_tokens, st.finished, st.all_done)), 50, 4 * V * d),
            'generate_32': (lambda: m.generate(None, prompt, 32, eos=eos, pad=pad, encoder_output=enc), 1, 0),
            'generate_128': (lambda: m.generate(None, prompt, 128, eos=eos, pad=pad, encoder_output=enc), 1, 0),
            'generate_128_eager': (lambda: m.generate(None, prompt, 128, eos=eos, pad=pad, encoder_output=enc, graph=False), 1, 0),
            'torch_encode': (lambda: tw.encode(feats), 2, 0),
            'torch_cross_kv': (lambda: tw.cross(enc), 2, 0),
            'torch_generate_32': (lambda: tw.generate(enc, prompt, 32, eos, pad), 1, 0),
            'torch_generate_128': (lambda: tw.generate(enc, prompt, 128, eos, pad), 1, 0),
        }
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, (fn, calls, _) in cases.items():
                times[k].append(timed(fn, calls))
        for k, (_, _, nbytes) in cases.items():
            res[k + '_us'] = round(statistics.median(times[k]), 1)
            res[k + '_us_min_max'] = [round(min(times[k]), 1), round(max(times[k]), 1)]
            if nbytes:
                res[k + '_gbs'] = round(nbytes / statistics.median(times[k]) / 1e3, 1)
        per_token = 4 * (nl * (6 * d * d + 2 * d * ffn) + V * d)      # per layer: self q|k|v and out 4 d^2, cross q and out 2 d^2, the MLP 2 d ffn; the tied projection
        res['step_weight_bytes'] = per_token
        res['step_graph_gbs'] = round(per_token / res['step_graph_us'] / 1e3, 1)
        res['hbm_copy_gbs'] = HBM_GBS
        for n in ('encode', 'cross_kv', 'generate_32', 'generate_128'):
            res[f'torch_over_hip_{n}'] = round(res[f'torch_{n}_us'] / res[f'{n}_us'], 2)
        print(json.dumps(res), flush=True)
        del st, graph


if __name__ == '__main__':
    main()
