"""varhip_code_table_f32 and varhip_rans_decode_u32 against their host twins, bit for bit (the twins are pinned against Python integers in
tests/test_codec_cpu.py).  Every device call runs through tests/util.guarded_call: operands inside guard bands."""
import numpy as np
import pytest
import torch

from tests import test_codec_cpu as H
from tests import util

pytestmark = pytest.mark.gpu

NAN_U32 = 0x7FC00000


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.view(dtype))).cuda()


def gpu_table(logits, B, l, V, t=0.0, t_rows=None, gt=None, ld=None, want_cum=True):
    ld = l if ld is None else ld
    cum = torch.full((B * l, V), NAN_U32, dtype=torch.int32, device='cuda') if want_cum else None      # a NaN pattern: every entry must be written
    pairs = torch.full((B, ld, 2), -1515870811, dtype=torch.int32, device='cuda') if gt is not None else None
    flags = torch.full((B, ld), -77, dtype=torch.int32, device='cuda')
    tr = None if t_rows is None else torch.tensor(t_rows, dtype=torch.float64, device='cuda')
    util.guarded_call('code_table_f32', dev(logits), B, l, V, float(t), tr, dev(gt), ld, cum, pairs, flags)
    u = lambda x: None if x is None else x.cpu().numpy().view(np.uint32)
    return u(cum), u(pairs), flags.cpu().numpy()


def special_rows(logits, l, V):
    """what tests/test_codec_cpu.py puts into single rows: -inf entries, all equal, one dominant entry, ties at the maximum, refused rows"""
    logits[0, ::3] = -np.inf
    logits[1 % l] = 0.375
    if l >= 9:
        logits[2] = -50.0; logits[2, 77] = 60.0
        logits[3, 200] = logits[3, 9] = logits[3, 130] = logits[3].max() + 2.0
        logits[4, 5] = np.nan
        logits[5, 6] = np.inf
        logits[6] = -np.inf
        logits[7, V - 1] = logits[7].max() + 1.0                        # v* in the row's last float4


@pytest.mark.parametrize('V', [256, 4096, 8192])
@pytest.mark.parametrize('B, l', [(1, 1), (3, 9)])
@pytest.mark.parametrize('mode', ['scalar', 'rows', 'zero'])
def test_code_table_equals_its_host_twin(V, B, l, mode):
    logits = H.make_logits(B, l, V, seed=V + 31 * B + l)
    if mode == 'zero':
        special_rows(logits, l, V)
    t_rows = [0.25, 1.5, 3.0][:B] if mode == 'rows' else None
    t = 0.0 if mode == 'zero' else 1.25
    ld = l + 3
    gt = np.full((B, ld), -5, np.int64)
    gt[:, :l] = np.random.default_rng(7).integers(0, V, (B, l))
    if l >= 9:
        gt[0, 2], gt[0, 3], gt[0, 7], gt[0, 8] = 77, 9, V - 1, V         # the dominant entry, v* of a tie, the last code, an id past the row
    want = H.host_table(logits, B, l, V, t, t_rows, gt, ld)
    got = gpu_table(logits, B, l, V, t, t_rows, gt, ld)
    for name, g, w in zip(('cum', 'pairs', 'flags'), got, want):
        ok, msg = util.diff_report(name, g[:, :l] if name != 'cum' else g, w[:, :l] if name != 'cum' else w)
        assert ok, msg
    assert (got[2][:, l:] == -77).all() and (got[1][:, l:] == 0xA5A5A5A5).all(), 'only the (B, l) corner is written'
    if mode == 'zero' and l >= 9:
        assert got[2][0].tolist()[:9] == [0, 0, 0, 0, 1, 1, 1, 0, 2]
    cum1, _, f1 = gpu_table(logits, B, l, V, t, t_rows, None, ld)                    # each output with the other NULL: the same bits
    _, pairs2, f2 = gpu_table(logits, B, l, V, t, t_rows, gt, ld, want_cum=False)
    assert np.array_equal(cum1, got[0]) and np.array_equal(pairs2, got[1]) and np.array_equal(f2, got[2])
    assert np.array_equal(f1[:, :l] != 0, (got[2][:, :l] == 1))


def test_code_table_einval():
    from var_amd import abi, hip
    V = 256
    x = torch.zeros(2 * 2 * V + 4, dtype=torch.float32, device='cuda')
    cum, flags = torch.zeros(2 * V + 4, dtype=torch.int32, device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda')
    fn = hip.lib().fn['code_table_f32']
    P = lambda a: None if a is None else a.data_ptr()
    for a in ((P(x[1:]), 1, 2, V, 0.0, None, None, 2, P(cum), None, P(flags)),         # logits not 16-byte aligned
              (P(x), 1, 2, V, 0.0, None, None, 2, P(cum[1:]), None, P(flags)),          # cum_out not 16-byte aligned
              (P(x), 1, 2, V, 0.0, None, None, 2, None, None, P(flags)),                # no output
              (P(x), 1, 2, 320, 0.0, None, None, 2, P(cum), None, P(flags)),
              (P(x), 1, 2, V, 0.0, None, None, 1, P(cum), None, P(flags))):
        assert fn(*a, None) == abi.EINVAL, a
    torch.cuda.synchronize()


def _streams(V, n, seed, shifts=(0, 1, 2)):
    """per image: (symbols, stream) with symbol i of image b under table (b + i) % 16 of a pool -> (pool of cumulative tables, ...)"""
    tabs = H._pool(V, 'random', seed=seed)
    cums = np.array([H.R.cumulative(F) for F in tabs], np.uint32)
    syms, streams = [], []
    for b in shifts:
        s = H._symbols(tabs, n, ['random', 'most', 'least'][b], 40 + b, shift=b)
        C = np.array([int(cums[(b + i) % 16][v - 1]) if v else 0 for i, v in enumerate(s)], np.int64)
        Fs = np.array([int(cums[(b + i) % 16][v]) for i, v in enumerate(s)], np.int64) - C
        syms.append(s); streams.append(H.host_encode(np.stack([C, Fs], 1)))
    rows = lambda lo, hi: np.concatenate([cums[(b + np.arange(lo, hi)) % 16] for b in shifts])
    return syms, streams, rows


def gpu_decode(cum, l, V, streams, state=None, err=None):
    B = len(streams)
    words = np.concatenate(streams).astype(np.uint32)
    nw = np.array([len(s) for s in streams], np.int64)
    off = np.concatenate(([0], np.cumsum(nw)[:-1])).astype(np.int64)
    state = torch.zeros(B, 4, dtype=torch.int32, device='cuda') if state is None else state
    err = torch.zeros(B, dtype=torch.int32, device='cuda') if err is None else err
    idx = torch.full((B, l), -77, dtype=torch.int64, device='cuda')
    util.guarded_call('rans_decode_u32', dev(cum, np.int32), l, V, dev(words, np.int32), int(words.size), dev(off), dev(nw), state, idx, err, B)
    return idx, state, err


@pytest.mark.parametrize('V', [256, 4096])
@pytest.mark.parametrize('B', [1, 3])
def test_rans_decode_equals_its_host_twin_across_two_scales(V, B):
    """l = 1, then l = 25, the state carried in `state`; streams of different lengths"""
    n = 26
    syms, streams, rows = _streams(V, n, seed=5, shifts=tuple(range(B)))
    assert len({len(s) for s in streams}) == B
    hs = H.host_decode(rows(0, 1), 1, V, streams)
    h1 = H.host_decode(rows(1, n), n - 1, V, streams, hs[1].copy(), hs[2].copy())
    g0 = gpu_decode(rows(0, 1), 1, V, streams)
    assert np.array_equal(g0[0].cpu().numpy(), hs[0]) and np.array_equal(g0[1].cpu().numpy().view(np.uint32), hs[1])
    g1 = gpu_decode(rows(1, n), n - 1, V, streams, g0[1], g0[2])
    assert np.array_equal(g1[0].cpu().numpy(), h1[0]) and np.array_equal(g1[1].cpu().numpy().view(np.uint32), h1[1])
    assert np.array_equal(g1[2].cpu().numpy(), h1[2]) and not h1[2].any()
    for b in range(B):
        assert g0[0][b].tolist() + g1[0][b].tolist() == syms[b] and H.end_ok(h1[1][b], h1[2][b], len(streams[b]))


@pytest.mark.parametrize('how', ['truncated', 'flipped', 'zero table'])
def test_one_corrupt_image_of_three(how):
    """the corrupt image's tokens are -1 from the bad word on and its err is set; its neighbours decode as if alone; in the next scale the
    image stays -1"""
    V, n = 256, 60
    syms, streams, rows = _streams(V, n, seed=11, shifts=(0, 2, 1))      # image 1: the longest stream
    assert len(streams[1]) > 20
    bad = list(streams)
    cum = rows(0, n).copy()
    if how == 'truncated':
        bad[1] = streams[1][:4]
    elif how == 'flipped':
        bad[1] = streams[1].copy(); bad[1][10] ^= 0x00400000
    else:
        cum[n + 7] = 0                                                  # a refused row: token 7 of image 1
    h = H.host_decode(cum, n, V, bad)
    g = gpu_decode(cum, n, V, bad)
    assert np.array_equal(g[0].cpu().numpy(), h[0]) and np.array_equal(g[2].cpu().numpy(), h[2])
    assert np.array_equal(g[1].cpu().numpy().view(np.uint32), h[1])
    idx = g[0].cpu().numpy()
    assert idx[0].tolist() == syms[0] and idx[2].tolist() == syms[2] and h[2][0] == 0 and h[2][2] == 0
    assert not H.end_ok(h[1][1], h[2][1], len(bad[1]))
    if how != 'flipped':
        assert h[2][1] == (1 if how == 'truncated' else 2)
        first = int(np.argmax(idx[1] == -1))
        assert (idx[1, first:] == -1).all() and idx[1, :first].tolist() == syms[1][:first] and (how != 'zero table' or first == 7)
        g2 = gpu_decode(cum, n, V, bad, g[1], g[2])
        assert (g2[0][1] == -1).all() and int(g2[2][1]) == int(h[2][1])
