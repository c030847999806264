"""CPU: the host-side layer of the operator wrappers (td-vc-gan_amd/_host.py): which layouts reach a kernel as views and which as
dense copies, the strides reported for them, the autograd path of the YIN flavour, the shape and device errors, the per-row
lengths and parameter vectors, and the table cache. Pure torch stride logic: no GPU and no built library."""
import importlib

import numpy as np
import pytest
import torch

from common import pkg

B, T = 3, 5
N, D = 4, 2


def host():
    pkg()
    return importlib.import_module('td-vc-gan_amd._host')


def as_kernel_reads(t, shape, strides):
    """What a kernel makes of (data_ptr, strides): the elements at those offsets from t's first element."""
    return torch.as_strided(t, shape, strides)


def numbered(*shape):
    return torch.arange(float(np.prod(shape))).reshape(shape)


ROW_VIEWS = {
    'contiguous': lambda: numbered(B, T),
    '[T]': lambda: numbered(T),
    '[B, 1, T]': lambda: numbered(B, 1, T),
    '[B, 1, T] of a wider buffer': lambda: numbered(B, 11)[:, None, 2:7],
    'row-strided slice': lambda: numbered(B, 11)[:, 2:7],
    'every other row': lambda: numbered(2 * B, T)[::2],
    'expanded row': lambda: numbered(T)[None].expand(B, T),
}


@pytest.mark.parametrize('name', sorted(ROW_VIEWS))
def test_rows2_views(name):
    H = host()
    x = ROW_VIEWS[name]()
    x2, bs, lead = H.rows2('op', x)
    want = x.reshape(-1, T)
    rows = want.shape[0]
    assert x2.data_ptr() == x.data_ptr(), 'a copy'
    assert x2.shape == (rows, T) and torch.equal(x2, want) and lead == tuple(x.shape[:-1])
    assert x2.stride(1) == 1 and bs == (x2.stride(0) if rows > 1 else T)
    assert torch.equal(as_kernel_reads(x2, (rows, T), (bs, 1)), want)
    if name == 'expanded row':
        assert bs == 0
    # the [..., T] rule takes the same layouts the same way
    y2, ybs, ylead = H.rows2('op', x, any_lead=True)
    assert y2.data_ptr() == x.data_ptr() and ybs == bs and ylead == lead and torch.equal(y2, want)


def test_rows2_single_row_reports_T():
    H = host()
    wide = numbered(B, 11)
    for x in (wide[1:2, 2:7], wide[1:2, None, 2:7], wide[1, 2:7]):
        x2, bs, _ = H.rows2('op', x)
        assert x2.data_ptr() == x.data_ptr() and x2.shape == (1, T) and bs == T      # not stride(0) = 11


def test_rows2_copies_a_non_dense_last_axis():
    H = host()
    x = numbered(B, 2 * T)[:, ::2]
    x2, bs, lead = H.rows2('op', x)
    assert x2.data_ptr() != x.data_ptr() and x2.is_contiguous() and bs == T and lead == (B,)
    assert torch.equal(x2, x)
    x2, bs, _ = H.rows2('op', numbered(B, 1, 2 * T)[:, :, ::2])
    assert x2.is_contiguous() and bs == T and torch.equal(x2, x)


def test_rows2_leading_axes():
    H = host()
    x = numbered(2, B, T)
    x2, bs, lead = H.rows2('yin_f0', x, any_lead=True)
    assert x2.data_ptr() == x.data_ptr() and x2.shape == (2 * B, T) and bs == T and lead == (2, B)
    x2, bs, lead = H.rows2('yin_f0', x.transpose(0, 1), any_lead=True)      # no common stride: reshape copies
    assert lead == (B, 2) and torch.equal(x2, x.transpose(0, 1).reshape(-1, T)) and bs == x2.stride(0)
    x2, bs, lead = H.rows2('op', torch.zeros(0, 1, T))
    assert x2.shape == (0, T) and bs == T and lead == (0, 1)
    x2, bs, lead = H.rows2('op', torch.zeros(B, 1, 0))
    assert x2.shape == (B, 0) and lead == (B, 1)
    assert H.rows2('op', numbered(B, T).double())[0].dtype == torch.float32
    assert H.rows2('op', torch.arange(T))[0].dtype == torch.float32


def test_rows2_autograd():
    H = host()
    leaf = numbered(B, 11).requires_grad_()
    x2, bs, _ = H.rows2('yin_f0', leaf[:, 2:7], any_lead=True, keep_grad=True)
    assert x2.requires_grad and bs == 11
    x2.sum().backward()
    want = torch.zeros(B, 11)
    want[:, 2:7] = 1.0
    assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, want)
    leaf3 = numbered(B, 1, 2 * T).requires_grad_()                                      # through the copy of a non-dense axis too
    x2, _, _ = H.rows2('yin_f0', leaf3[:, :, ::2], any_lead=True, keep_grad=True)
    (2.0 * x2).sum().backward()
    assert leaf3.grad.shape == (B, 1, 2 * T) and torch.equal(leaf3.grad[0, 0], torch.tensor([2.0, 0.0] * T))
    assert not H.rows2('op', leaf)[0].requires_grad                                      # detached unless asked


def test_rows2_shape_errors_name_the_caller():
    H = host()
    for bad in (torch.zeros(B, 2, T), torch.zeros(2, B, 1, T), torch.zeros(())):
        with pytest.raises(ValueError, match='sos_filter'):
            H.rows2('sos_filter', bad)
    with pytest.raises(ValueError, match='yin_f0'):
        H.rows2('yin_f0', torch.zeros(()), any_lead=True)


FRAME_VIEWS = {
    'contiguous': lambda: numbered(B, N, D),
    '[N, D]': lambda: numbered(N, D),
    'slice of a wider buffer': lambda: numbered(B, N + 2, D + 2)[:, 1:1 + N, :D],
    'every other pair': lambda: numbered(2 * B, N, D)[::2],
    'every other frame': lambda: numbered(B, 2 * N, D)[:, ::2],
    'expanded pair': lambda: numbered(N, D)[None].expand(B, N, D),
    '[2, B, N, D]': lambda: numbered(2, B, N, D),
}


@pytest.mark.parametrize('name', sorted(FRAME_VIEWS))
def test_frames3_views(name):
    H = host()
    t = FRAME_VIEWS[name]()
    t3, bs, fs = H.frames3('op', t)
    want = t.reshape(-1, N, D)
    pairs = want.shape[0]
    assert t3.data_ptr() == t.data_ptr(), 'a copy'
    assert t3.shape == (pairs, N, D) and torch.equal(t3, want)
    assert t3.stride(2) == 1 and fs == t3.stride(1) and bs == (t3.stride(0) if pairs > 1 else N * D)
    assert torch.equal(as_kernel_reads(t3, (pairs, N, D), (bs, fs, 1)), want)
    if name == 'expanded pair':
        assert bs == 0


def test_frames3_single_pair_and_single_frame():
    H = host()
    t3, bs, fs = H.frames3('op', numbered(N, D))
    assert (bs, fs) == (N * D, D)
    wide = numbered(B, N + 2, D + 2)
    t3, bs, fs = H.frames3('op', wide[1:2, 1:1 + N, :D])          # one pair of a wider buffer: its frames are still D + 2 apart
    assert t3.data_ptr() == wide[1:2, 1:1 + N, :D].data_ptr() and (bs, fs) == (N * D, D + 2)
    t3, bs, fs = H.frames3('op', wide[:, 1:2, :D])                # one frame per pair reports D
    assert t3.shape == (B, 1, D) and (bs, fs) == ((N + 2) * (D + 2), D)


def test_frames3_dense_copies():
    H = host()
    cases = {'non-dense last axis': numbered(B, N, 2 * D)[:, :, ::2],
             'expanded frames': numbered(B, 1, D).expand(B, N, D),             # frame stride 0 < D
             'overlapping frames': torch.as_strided(numbered(B * (N + 1)), (B, N, D), (N + 1, 1, 1))}
    for name, t in cases.items():
        t3, bs, fs = H.frames3('op', t)
        assert t3.is_contiguous() and (bs, fs) == (N * D, D) and torch.equal(t3, t), name
        assert t3.data_ptr() != t.data_ptr(), name
    assert H.frames3('op', numbered(B, N, D).double())[0].dtype == torch.float32
    assert not H.frames3('op', numbered(B, N, D).requires_grad_())[0].requires_grad


def test_frames3_shape_errors_name_the_caller():
    H = host()
    for bad in (torch.zeros(D), torch.zeros(())):
        with pytest.raises(ValueError, match='viterbi_path'):
            H.frames3('viterbi_path', bad)


def test_need_device_has_no_cpu_fallback():
    H = host()
    Err = pkg()._lib.TdvcError
    for bad in ((torch.zeros(T),), (None,), (np.zeros(T),), (torch.zeros(T), 3.0)):
        with pytest.raises(Err, match='no CPU fallback') as e:
            H.need_device('resample', *bad)
        assert 'resample' in str(e.value)
    H.need_device('resample')                                      # nothing to check


def test_device_lengths_strict():
    """What speaker and ecapa take: None stays None, a tensor must be on a device already, the shape is (B,)."""
    H = host()
    Err = pkg()._lib.TdvcError
    assert H.device_lengths('fbank', None, B, 'cpu') is None
    assert H.device_lengths('fbank', None, B, 'cpu', move=True, any_shape=True) is None
    for bad in (torch.tensor([5, 4, 3]), torch.tensor([5, 4, 3, 2]), torch.tensor([[5], [4], [3]])):
        with pytest.raises(Err, match='no CPU fallback') as e:                           # before any shape check
            H.device_lengths('fbank', bad, B, 'cpu')
        assert 'fbank' in str(e.value)


def test_device_lengths_moving():
    """What evaluate and pitch take: a tensor on another device is moved, the values arrive as int32 [B], contiguous."""
    H = host()
    want = torch.tensor([5, 0, 3], dtype=torch.int32)
    wide = torch.tensor([5, 9, 0, 9, 3, 9])
    cases = {'list': [5, 0, 3], 'tuple': (5, 0, 3), 'numpy': np.array([5, 0, 3]), 'int64 tensor': torch.tensor([5, 0, 3]),
             'int32 tensor': want.clone(), 'strided view': wide[::2]}
    for name, v in cases.items():
        for kw in ({'move': True}, {'move': True, 'any_shape': True}):
            r = H.device_lengths('dtw', v, B, 'cpu', **kw)
            assert r.dtype == torch.int32 and r.shape == (B,) and r.is_contiguous() and r.stride() == (1,) and torch.equal(r, want), name
    assert torch.equal(wide, torch.tensor([5, 9, 0, 9, 3, 9]))                           # the caller's tensor is left alone
    big = H.device_lengths('dtw', torch.tensor([2 ** 31 - 1, 0, 1]), B, 'cpu', move=True)
    assert big.tolist() == [2 ** 31 - 1, 0, 1]


def test_device_lengths_shapes():
    H = host()
    for bad in ([5, 4], [5, 4, 3, 2], torch.tensor([5, 4]), torch.zeros(B + 1, dtype=torch.int64), torch.tensor(5)):
        for kw in ({'move': True}, {'move': True, 'any_shape': True}):
            with pytest.raises(ValueError, match='dio') as e:
                H.device_lengths('dio', bad, B, 'cpu', **kw)
            assert f'[{B}]' in str(e.value)
    col = torch.tensor([[5], [0], [3]])
    for v in (col, col.tolist(), col.reshape(1, B), torch.tensor([5, 9, 0, 9, 3, 9]).reshape(B, 2)[:, :1]):
        r = H.device_lengths('dio', v, B, 'cpu', move=True, any_shape=True)
        assert r.shape == (B,) and r.dtype == torch.int32 and r.is_contiguous() and r.tolist() == [5, 0, 3]
        with pytest.raises(ValueError, match='dio'):                                     # the default wants [B] itself
            H.device_lengths('dio', v, B, 'cpu', move=True)


def test_vec():
    """A CPU has no device tensor to flatten: what can be pinned here is that nothing else gets through, and what the message names."""
    H = host()
    Err = pkg()._lib.TdvcError
    for bad in (torch.zeros(4), torch.zeros(2, 2), None, np.zeros(4), [0.0] * 4):
        with pytest.raises(Err, match='no CPU fallback') as e:
            H.vec('layer_norm', bad, 4, 'gamma')
        assert 'layer_norm' in str(e.value)
    with pytest.raises(Err):                                                             # the device check comes before the count
        H.vec('layer_norm', torch.zeros(5), 4)


def test_dft_tables():
    H = host()
    n = 8
    i = np.arange(n, dtype=np.float64)
    t = H.dft_tables(n, (0.54, 0.46))
    assert t.dtype == np.float64 and t.shape == (3 * n,)
    assert np.array_equal(t[:n], np.cos(2.0 * np.pi * i / n)) and np.array_equal(t[n:2 * n], np.sin(2.0 * np.pi * i / n))
    assert np.array_equal(t[2 * n:], 0.54 - 0.46 * np.cos(2.0 * np.pi * i / n))
    w = np.linspace(0.0, 1.0, n)
    for given in (w, w.tolist(), w.astype(np.float32)):
        u = H.dft_tables(n, given)
        assert u.dtype == np.float64 and np.array_equal(u[:2 * n], t[:2 * n]) and np.array_equal(u[2 * n:], np.asarray(given, dtype=np.float64))
    for bad in (w[:-1], (0.5, 0.5, 0.5)):
        with pytest.raises(ValueError):
            H.dft_tables(n, bad)
    P = pkg()
    for tab, fb, win in ((P.speaker, P.speaker.mel_filterbank(), (0.5, 0.5)), (P.ecapa, P.ecapa.fbank_matrix(16), (0.54, 0.46))):
        assert fb.shape[1] == 201 and H.dft_tables(tab.N_FFT, win).shape == (1200,)


def test_small_helpers():
    H = host()
    assert H.ptr(None) is None
    t = torch.zeros(3)
    assert H.ptr(t) == t.data_ptr()
    for n in (0, 1, 100):
        s = H.scratch(n, 'cpu')
        assert s.dtype == torch.uint8 and s.numel() == max(n, 1)
    assert H.dev_key('cpu') == H.dev_key(torch.device('cpu')) == ('cpu', None)
    assert H.dev_key('cuda:1') == H.dev_key(torch.device('cuda', 1)) == ('cuda', 1)
    H.check('op', 0)


def test_table_cache():
    H = host()
    calls = []

    def builder(tag, n):
        def build():
            calls.append(tag)
            a = np.arange(n, dtype=np.float64)
            a.setflags(write=False)
            return a
        return build
    cpu = torch.device('cpu')
    ka, kb = ('test_host_layout', 'a'), ('test_host_layout', 'b')
    a1 = H.device_table(cpu, ka, builder('a', 4))
    a2 = H.device_table('cpu', ka, builder('a', 4))
    assert a1 is a2 and calls == ['a']
    assert a1.dtype == torch.float64 and a1.tolist() == [0.0, 1.0, 2.0, 3.0]
    host_a = H.host_table(ka, builder('a', 4))                     # the host side of the same key: built already
    assert calls == ['a'] and isinstance(host_a, np.ndarray) and H.host_table(ka, builder('a', 4)) is host_a
    b1 = H.device_table(cpu, kb, builder('b', 2))
    assert calls == ['a', 'b'] and b1 is not a1 and b1.tolist() == [0.0, 1.0] and H.device_table(cpu, ka, builder('a', 4)) is a1

    def failing():
        calls.append('x')
        raise ValueError('no such table')
    for _ in range(2):                                             # a build that raises caches nothing
        with pytest.raises(ValueError):
            H.device_table(cpu, ('test_host_layout', 'x'), failing)
    assert calls == ['a', 'b', 'x', 'x']
    up = H.device_table(cpu, ('test_host_layout', 'pair'), builder('p', 3), lambda h, device: (torch.tensor(h * 2, device=device), len(h)))
    assert up[1] == 3 and up[0].tolist() == [0.0, 2.0, 4.0] and calls[-1] == 'p'


def test_wrappers_keep_their_host_side_entry_points():
    """The cached host tables stay reachable under their names, and the wrappers' checks run before anything touches a device."""
    P = pkg()
    m = P.evaluate.sp2mc_matrix(16, 4)
    assert P.evaluate.sp2mc_matrix(16, 4) is m and m.shape == (5, 9) and not m.flags.writeable
    g = P.evaluate.cheaptrick_mc_matrix(16, 4)
    assert P.evaluate.cheaptrick_mc_matrix(16, 4) is g and g.shape == (5, 9) and not np.array_equal(g, m)
    for fn in (P.evaluate.sp2mc_matrix, P.evaluate.cheaptrick_mc_matrix):
        with pytest.raises(ValueError, match=fn.__name__):
            fn(15)
    logw, lo = P.pitch._transition_host(32, 266, 240.0)
    assert P.pitch._transition_host(32, 266, 240.0)[0] is logw and logw.shape[0] == lo.shape[0] == 233
    Err = P._lib.TdvcError
    x = torch.zeros(B, 1, 64)
    for call in (lambda: P.pitch.yin_f0(x[:, 0], 16000), lambda: P.pitch.viterbi_path(torch.zeros(4, 3), None, None),
                 lambda: P.corrupt.sos_filter(x, torch.zeros(B, 1, 6)), lambda: P.resample.resample(x, 48000, 16000),
                 lambda: P.evaluate.dtw(x, x), lambda: P.evaluate.mel_cepstrum(x), lambda: P.evaluate.cheaptrick(x, torch.zeros(B, 2)),
                 lambda: P.util.f0_to_excitation(x, 64)):
        with pytest.raises(Err, match='no CPU fallback'):
            call()
