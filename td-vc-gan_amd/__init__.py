"""tdvc-mi355x: MI355X-native (gfx950) implementation of TD-VC-GAN's G+D train-step path.

Drop-in surface (same names / signatures / state_dict keys as the reference):
    Generator, CollaborativeMultibandDiscriminator, ConditionalInstanceNorm, LatentClassifier,
    losses.{multiscale_spec_loss, multiscale_feat_loss, contrastive_loss}, TrainStep, and the YIN pitch tracker of util/yin.py as
    yin_f0 / track_f0 (pitch.py; decoder='viterbi' with viterbi_transition / viterbi_path is the temporal decoding of the
    inference scripts), and the data pipeline's signal corruption (data/dataset.py corrupt_audio: a random parametric
    EQ, RMS-matched) as corrupt_audio / random_eq / sos_filter / peq_sos, with device_batch for the whole batch dict (corrupt.py), and
    load_audio's resampling and segment preparation as resample / load_segments (resample.py), and the objective evaluation of
    test_scripts/common/test_mcd.py as mcd / dtw / fastdtw / mel_cepstrum / sp2mc / sp2mc_matrix / f0_stats, with WORLD's CheapTrick envelope as cheaptrick (evaluate.py)
    and WORLD's DIO + StoneMask F0 as dio / stonemask / world_f0 (pitch.py; mcd(f0_method='dio')), and the speaker-similarity
    evaluation of test_scripts/common/test_speaker_rec.py (Resemblyzer's VoiceEncoder.embed_utterance, per-speaker centroids, cosine
    similarity and nearest-centroid accuracy) as VoiceEncoder / load_voice_encoder / voice_mel / lstm_fwd / partial_slices /
    window_count / speaker_similarity (speaker.py), and the speechbrain speaker recognition of
    test_scripts/mls-pt/test_speaker_rec.py (Fbank features, the ECAPA-TDNN embedding, the cosine classifier) as EcapaTdnn /
    load_ecapa / fbank / fbank_matrix / speaker_classify / running_mean_norm (ecapa.py), and the WavLM feature extractor that
    model/ssl_encoder.py injects into SSLEncoder (wavlm/WavLM.py extract_features) as WavLM / WavLMConfig / load_wavlm (wavlm.py), and
    the CREPE pitch tracker of util/crepe.py (torchcrepe's tiny / full network, its front end and its argmax, weighted-argmax and
    Viterbi decoders) as Crepe / load_crepe / crepe_frames / crepe_decode / crepe_transition / get_shift (crepe.py), and the
    activation-MSE F0 term of train.py:439-470 on it as losses.f0_crepe_loss / activation_mse / Crepe.activations_with_grad, with the
    target of train.py:245-252 as conversion_target / roll_bins (StepConfig.f0_loss='activation'), and the intelligibility metric
    of test_scripts/common/test_asr.py (Whisper's log-mel features, encoder and greedy decoder, WER / CER) as Whisper / WhisperConfig /
    load_whisper / whisper_log_mel / asr_wer / asr_cer / asr_report (whisper.py).

The HIP library (csrc/ -> libtdvc_hip.so, C ABI in include/tdvc.h) is loaded lazily on the first
operator call and the load fails loudly when it is missing: there is no CPU or ATen fallback in
the product path. The directory name contains hyphens; import it as `import tdvc_amd` (alias
module at the repo root) or `importlib.import_module('td-vc-gan_amd')`.
"""
__version__ = '0.1.0'

from . import synth  # noqa: F401  (numpy/torch only, no GPU)


def __getattr__(name):
    # heavy submodules on demand, so that `synth` stays importable without torch.cuda / the .so
    import importlib
    if name in ('modules', 'losses', 'ops', 'arena', 'train_step', 'parallel', 'hparams', 'util', 'infer', 'ssl_encoder', 'pitch', 'corrupt', 'resample', 'evaluate', 'speaker', 'ecapa', 'wavlm', 'crepe', 'whisper', '_lib'):
        return importlib.import_module(f'{__name__}.{name}')
    if name in ('Generator', 'CollaborativeMultibandDiscriminator', 'ConditionalInstanceNorm', 'LatentClassifier', 'Discriminator'):
        return getattr(importlib.import_module(f'{__name__}.modules'), name)
    if name in ('yin_f0', 'track_f0', 'viterbi_transition', 'viterbi_path', 'dio', 'stonemask', 'world_f0'):
        return getattr(importlib.import_module(f'{__name__}.pitch'), name)
    if name in ('peq_sos', 'sos_filter', 'random_eq', 'corrupt_audio', 'device_batch'):
        return getattr(importlib.import_module(f'{__name__}.corrupt'), name)
    if name in ('resample_filter', 'resample_bank', 'load_segments'):      # `resample` is the (callable) module itself, above
        return getattr(importlib.import_module(f'{__name__}.resample'), name)
    if name in ('dtw', 'fastdtw', 'mcd','f0_stats', 'sp2mc', 'sp2mc_matrix', 'mel_cepstrum', 'cheaptrick', 'cheaptrick_mc_matrix'):
        return getattr(importlib.import_module(f'{__name__}.evaluate'), name)
    if name in ('VoiceEncoder', 'load_voice_encoder', 'voice_mel', 'lstm_fwd', 'partial_slices', 'window_count', 'speaker_similarity'):
        return getattr(importlib.import_module(f'{__name__}.speaker'), name)
    if name in ('EcapaTdnn', 'load_ecapa', 'fbank', 'fbank_matrix', 'speaker_classify', 'running_mean_norm'):
        return getattr(importlib.import_module(f'{__name__}.ecapa'), name)
    if name in ('WavLM', 'WavLMConfig', 'load_wavlm'):
        return getattr(importlib.import_module(f'{__name__}.wavlm'), name)
    if name in ('Crepe', 'load_crepe', 'crepe_frames', 'crepe_conv', 'crepe_head', 'crepe_decode', 'crepe_lattice', 'crepe_transition', 'get_shift',
                'crepe_conv_bwd', 'crepe_head_bwd', 'crepe_frames_bwd', 'crepe_act_mse', 'pack_bwd_weight', 'roll_bins', 'conversion_target',
                'activation_mse'):
        return getattr(importlib.import_module(f'{__name__}.crepe'), name)
    if name in ('Whisper', 'WhisperConfig', 'load_whisper', 'whisper_log_mel', 'whisper_mel_filters', 'asr_wer', 'asr_cer', 'asr_report'):
        return getattr(importlib.import_module(f'{__name__}.whisper'), name)
    if name in ('TrainStep', 'StepConfig'):
        return getattr(importlib.import_module(f'{__name__}.train_step'), name)
    raise AttributeError(name)
