"""Forward-only conversion path: what generate_with_target.py:54-184 does around the generator call, with the
same kernels as the train step — checkpoint interchange (`step{E}-G.pt` / `latest-G.pt` are plain state_dicts with the
reference's keys), F0 tracking on the device (YIN, pitch.py), log-F0 mean shift towards the target speaker, excitation on the
device, one whole-utterance forward.

`convert_audio` goes from waveform to waveform: `pitch.track_f0` -> F0 scaling -> `convert`, or with `f0_tracker=` a `crepe.Crepe`
the reference's own CREPE tracker (util/crepe.py filtered_pitch(signal, "viterbi")) in place of YIN. `convert` still takes an F0
track, so a caller with another tracker passes that track in. Audio I/O stays with the caller.
"""
import torch

from . import modules as M
from .pitch import track_f0
from .util import f0_to_excitation

SEGMENT_MULT = 320       # product of the decoder ratios (data/dataset.py:41): utterances are padded to a multiple of it
F0_HOP = 64


def build_generator(gen_cfg, num_spk, device):
    """Generator from the `model.generator` section of a reference config (train.py:125-138 argument order)."""
    g = gen_cfg
    nl, wn, cond = g['norm_layer'], g['weight_norm'], g['conditioning']
    G = M.Generator(list(g['decoder_ratios']), list(g['decoder_channels']), g['num_bottleneck_layers'], num_spk,
                    g['conditional_dim'], g['content_dim'], g['num_res_blocks'], g['num_enc_layers'], g['encoder_model'],
                    norm_layer=(nl['bottleneck'], nl['encoder'], nl['decoder']),
                    weight_norm=(wn['bottleneck'], wn['encoder'], wn['decoder']),
                    bot_cond=cond['bottleneck'], enc_cond=cond['encoder'], dec_cond=cond['decoder'])
    G.ensure_arena(device)
    return G


def load_generator_checkpoint(G, path):
    """Load a reference checkpoint (a state_dict saved by train.py:597-608). Nothing from the file is executed."""
    sd = torch.load(path, map_location='cpu', weights_only=True)
    G.load_state_dict(sd)      # copies into the arena-backed parameters in place
    return G


def shift_f0(f0_src, f0_tgt):
    """log-F0 mean shift of the source contour towards the target speaker (generate_with_target.py:135-160,
    train.py:245-251). f0: [B, 1, n] in Hz, 0 = unvoiced. Element-wise pre-processing on a few hundred frames."""
    def mu(f):
        v = f > 0
        return (v * torch.log(f + 1e-6)).sum(-1, keepdim=True) / (v.sum(-1, keepdim=True) + 1e-6)
    out = torch.zeros_like(f0_src)
    voiced = f0_src > 0
    out[voiced] = torch.exp(torch.log(f0_src + 1e-6) + mu(f0_tgt) - mu(f0_src))[voiced]
    return out


@torch.no_grad()
def convert(G, signal, c_tgt, f0_conv, noise=None, start_phase=None):
    """signal [1, 1, T] (T a multiple of 320, >= 8320), c_tgt one-hot [1, num_spk], f0_conv [1, 1, T/64 + 1] -> converted
    signal [1, 1, T]. One forward of the whole utterance, as the reference does (test.max_segment = 71680 samples)."""
    T = signal.shape[-1]
    if T % SEGMENT_MULT:
        raise ValueError(f'utterance length {T} is not a multiple of {SEGMENT_MULT} (pad it as data/dataset.py:158-163 does)')
    exc = f0_to_excitation(f0_conv, F0_HOP, noise=noise, start_phase=start_phase)
    if exc.shape[-1] != T:
        raise ValueError(f'F0 track gives {exc.shape[-1]} excitation samples for a {T}-sample utterance')
    return G(signal, c_tgt, c_var=exc)


@torch.no_grad()
def convert_audio(G, signal, c_tgt, f0_ratio=1.0, noise=None, start_phase=None, f0_tracker=None, target_signal=None, **track_kwargs):
    """Waveform in, waveform out: the F0 track of `signal` [1, 1, T] from `pitch.track_f0` (track_kwargs: hop, sample_rate, pitch_min,
    pitch_max, threshold, decoder, octave_cost, jump_cost), scaled by f0_ratio (the target / source mean-F0 ratio, train.py:636), then
    `convert`. decoder='viterbi' decodes the track over time, as the reference's inference scripts do (generate_with_target.py:139,
    util.crepe.filtered_pitch(signal, "viterbi")); the default is the per-frame decision. For the log-F0 mean shift instead, call
    `track_f0` on both speakers, `shift_f0`, and `convert`.
    f0_tracker: a `crepe.Crepe` replaces YIN by the reference's own tracker, `f0_tracker.filtered_pitch(signal, 'viterbi')`
    (generate_with_target.py:139); with `target_signal` [1, 1, T'] the target speaker's utterance is tracked the same way (:161) and
    the source contour gets the log-F0 mean shift of `shift_f0` towards it (:163-165) before f0_ratio is applied. track_kwargs belong
    to YIN and are refused with a tracker; target_signal needs one. With f0_tracker=None nothing changes."""
    if f0_tracker is None:
        if target_signal is not None:
            raise ValueError('convert_audio: target_signal needs f0_tracker (or call track_f0, shift_f0 and convert)')
        f0_conv = track_f0(signal, **track_kwargs) * f0_ratio
    else:
        if track_kwargs:
            raise ValueError(f'convert_audio: {sorted(track_kwargs)} are arguments of track_f0 and do not apply to f0_tracker')
        f0_conv, _ = f0_tracker.filtered_pitch(signal, 'viterbi')
        if target_signal is not None:
            f0_conv = shift_f0(f0_conv, f0_tracker.filtered_pitch(target_signal, 'viterbi')[0])
        f0_conv = f0_conv * f0_ratio
    return convert(G, signal, c_tgt, f0_conv, noise=noise, start_phase=start_phase)
