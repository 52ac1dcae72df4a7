"""The host twins of lossless token coding (include/var_hip.h; no GPU needed): varhip_code_table_host_f32 against the Python-integer restatement
of the table in tests/codecref.py, bit for bit; varhip_rans_encode_host / varhip_rans_decode_host against codecref's coder and against each
other; the stream-size bound; corrupt streams; every refusal.  Every call runs with its operands inside guard arenas (tests/util.py)."""
import numpy as np
import pytest

from tests import codecref as R
from tests import util

PB, TOTAL = R.PB, R.TOTAL


def _host(name):
    from var_amd import hip
    return hip.lib().host[name]


def host_table(logits, B, l, V, t=0.0, t_rows=None, gt=None, ld=None, want_cum=True, expect=0):
    """-> (cum (B*l, V) uint32 | None, pairs (B, ld, 2) uint32 | None, flags (B, ld) int32), outputs prefilled with a sentinel"""
    ld = l if ld is None else ld
    cum = np.full((B * l, V), 0xA5A5A5A5, np.uint32) if want_cum else None
    pairs = np.full((B, ld, 2), 0xA5A5A5A5, np.uint32) if gt is not None else None
    flags = np.full((B, ld), -77, np.int32)
    tr = None if t_rows is None else np.asarray(t_rows, np.float64)
    fn = _host('code_table_host_f32')
    rc = util.guarded_invoke('varhip_code_table_host_f32', [logits, B, l, V, float(t), tr, gt, ld, cum, pairs, flags], lambda *a: fn(*a))
    assert rc == expect, rc
    return cum, pairs, flags


def host_encode(pairs, cap=None, expect=0):
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    n = pairs.shape[0]
    cap = n + 2 if cap is None else cap
    words, nw = np.zeros(max(cap, 1), np.uint32), np.full(1, -1, np.int64)
    fn = _host('rans_encode_host')
    rc = util.guarded_invoke('varhip_rans_encode_host', [pairs if n else np.zeros((1, 2), np.uint32), n, words, cap, nw], lambda *a: fn(*a))
    assert rc == expect, rc
    return words[:int(nw[0])].copy() if rc == 0 else None


def host_decode(cum, l, V, streams, state=None, err=None):
    """streams: one uint32 array per image -> (idx (B, l), state (B, 4), err (B,))"""
    B = len(streams)
    words = np.concatenate(streams).astype(np.uint32) if sum(len(s) for s in streams) else np.zeros(0, np.uint32)
    nw = np.array([len(s) for s in streams], np.int64)
    off = np.concatenate(([0], np.cumsum(nw)[:-1])).astype(np.int64)
    state = np.zeros((B, 4), np.uint32) if state is None else state
    err = np.zeros(B, np.int32) if err is None else err
    idx = np.full((B, l), -77, np.int64)
    fn = _host('rans_decode_host')
    buf = words if words.size else np.zeros(1, np.uint32)
    rc = util.guarded_invoke('varhip_rans_decode_host', [cum, l, V, buf, int(words.size), off, nw, state, idx, err, B], lambda *a: fn(*a))
    assert rc == 0, rc
    return idx, state, err


def end_ok(state, err, nw):
    return int(err) == 0 and (int(state[0]) | int(state[1]) << 32) == R.LOW and int(state[2]) == nw


def make_logits(B, l, V, seed, scale=4.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((2 * B * l, V)) * scale).astype(np.float32)


def check_rows(logits, B, l, V, t_of_image, cum, pairs, flags, gt, ld):
    """the twin's outputs against codecref, bit for bit, and the table's invariants on the reference itself"""
    ref = R.tables(logits, B, l, t_of_image)
    rows = B * l
    for w, rt in enumerate(ref):
        b, j = divmod(w, l)
        if rt is None:
            assert flags[b, j] == 1 and (cum is None or not cum[w].any()) and (pairs is None or not pairs[b, j].any()), w
            continue
        F, vstar = rt
        assert sum(F) == TOTAL and min(F) >= 1, w
        z = R.guided(logits[w], logits[rows + w], t_of_image[b])
        # monotone: F_a >= F_b wherever z_a >= z_b, for every b that is not v* (v* alone carries the remainder D; with a = v* the claim holds
        # a fortiori).  In sorted order that is: F without v*'s D never decreases along ascending z.
        Fq = np.array(F, np.int64)
        order = np.argsort(z, kind='stable')
        assert (np.diff(Fq[order][order != vstar]) >= 0).all() and Fq[vstar] == Fq.max(), w
        assert flags[b, j] == 0, w
        if cum is not None:
            assert np.array_equal(cum[w], np.array(R.cumulative(F), np.uint32)), f'row {w}: cumulative table'
        if pairs is not None:
            g = int(gt[b, j])
            assert tuple(int(v) for v in pairs[b, j]) == (sum(F[:g]), F[g]), f'row {w}: pair'
    assert (flags[:, l:] == -77).all() and (pairs is None or (pairs[:, l:] == 0xA5A5A5A5).all()), 'only the (B, l) corner is written'


@pytest.mark.parametrize('V', [256, 4096, 8192])
@pytest.mark.parametrize('B, l', [(1, 1), (3, 9), (1, 9), (3, 1)])
@pytest.mark.parametrize('mode', ['scalar', 'rows', 'zero'])
def test_table_against_integer_reference(V, B, l, mode):
    logits = make_logits(B, l, V, seed=V + 31 * B + l)
    t_rows = [0.25, 1.5, 3.0][:B] if mode == 'rows' else None
    t = 0.0 if mode == 'zero' else 1.25
    ld = l + 3                                                          # a padded stride: a scale's slice of (B, L) tensors
    gt = np.full((B, ld), -5, np.int64)
    gt[:, :l] = np.random.default_rng(7).integers(0, V, (B, l))
    cum, pairs, flags = host_table(logits, B, l, V, t, t_rows, gt, ld)
    check_rows(logits, B, l, V, t_rows if t_rows is not None else [t] * B, cum, pairs, flags, gt, ld)


@pytest.mark.parametrize('V', [256, 4096, 8192])
def test_table_special_rows_and_single_outputs(V):
    """rows with -inf entries, all entries equal, one dominant entry (every other exponential is 0: F = 1), exact ties at the maximum (the
    remainder goes to the lowest index); each output alone gives the bits it gives beside the other"""
    B, l = 1, 5
    logits = make_logits(B, l, V, seed=3)
    logits[0, ::3] = -np.inf
    logits[1] = 0.375
    logits[2] = -50.0; logits[2, 77] = 60.0
    logits[3, 200] = logits[3, 9] = logits[3, 130] = logits[3].max() + 2.0
    gt = np.array([[1, V - 1, 77, 9, 0]], np.int64)
    cum, pairs, flags = host_table(logits, B, l, V, 0.0, None, gt)
    check_rows(logits, B, l, V, [0.0], cum, pairs, flags, gt, l)
    F = np.diff(np.concatenate(([0], cum[2].astype(np.int64))))
    assert (np.delete(F, 77) == 1).all() and F[77] == TOTAL - (V - 1)
    F = np.diff(np.concatenate(([0], cum[1].astype(np.int64))))
    assert F[0] == F[1] + (TOTAL - V) % V and (F[1:] == F[1]).all()    # all equal: q = K // V each, the remainder on index 0
    F = np.diff(np.concatenate(([0], cum[3].astype(np.int64))))
    assert F[9] >= F[130] == F[200]
    cum1, _, f1 = host_table(logits, B, l, V, 0.0, None, None)
    _, pairs2, f2 = host_table(logits, B, l, V, 0.0, None, gt, want_cum=False)
    assert np.array_equal(cum1, cum) and np.array_equal(pairs2, pairs) and np.array_equal(f1, flags) and np.array_equal(f2, flags)


@pytest.mark.parametrize('V', [256, 4096])
def test_table_close_to_float64_softmax(V):
    """F_v / 2^PB >= p64_v * (1 - 2^-11) - 2^-PB against the float64 softmax of the same fp32 z (derivation: DESIGN.md §32)"""
    B, l, t = 2, 4, 1.5
    for scale in (0.5, 4.0, 20.0):
        logits = make_logits(B, l, V, seed=int(scale * 10), scale=scale)
        cum, _, flags = host_table(logits, B, l, V, t)
        assert not flags.any()
        for w in range(B * l):
            z = R.guided(logits[w], logits[B * l + w], t).astype(np.float64)
            p = np.exp(z - z.max()); p /= p.sum()
            F = np.diff(np.concatenate(([0], cum[w].astype(np.int64))))
            assert (F / TOTAL >= p * (1 - 2.0 ** -11) - 2.0 ** -PB).all(), (scale, w)


def _pool(V, kind, seed=0):
    """16 tables (F lists) for the coder tests and per table the symbol the test codes: random, the most or the least probable"""
    rng = np.random.default_rng(seed)
    tabs = []
    for k in range(16):
        z = (rng.standard_normal(V) * (0.5 + k)).astype(np.float32)
        if kind == 'least':
            z[rng.integers(0, V)] = -np.inf                              # an F = 1 symbol for certain: 24 bits each
        tabs.append(R.table(z)[0])
    return tabs


def _symbols(tabs, n, kind, seed, shift=0):
    """n symbols, symbol i under table (shift + i) % 16"""
    if kind == 'random':
        return [int(v) for v in np.random.default_rng(seed).integers(0, len(tabs[0]), n)]
    pick = [int(np.argmax(F) if kind == 'most' else np.argmin(F)) for F in tabs]
    return [pick[(shift + i) % 16] for i in range(n)]


@pytest.mark.parametrize('kind', ['random', 'most', 'least'])
def test_round_trip_and_stream_size(kind):
    """n = 1 .. 700 symbols: decode(encode) returns the tokens, the end check holds, and 32 * nwords <= ideal bits + n / 64 + 64: every symbol
    costs at most log2(1 + 2^(PB - 31)) < 2^-6 bits over its ideal length (F / x <= 2^(PB - 31) at every encode step), the flush of the
    final state 64.  The streams of a few n are compared with codecref's word for word."""
    V = 256
    tabs = _pool(V, kind)
    cums = np.array([R.cumulative(F) for F in tabs], np.uint32)
    if kind == 'least':
        assert all(min(F) == 1 for F in tabs)
    for n in range(1, 701):
        syms = _symbols(tabs, n, kind, n)
        pairs = [(sum(tabs[i % 16][:s]), tabs[i % 16][s]) for i, s in enumerate(syms)] if n in (1, 2, 65, 700) else None
        C = np.array([int(cums[i % 16][s - 1]) if s else 0 for i, s in enumerate(syms)], np.int64)
        Fs = np.array([int(cums[i % 16][s]) for i, s in enumerate(syms)], np.int64) - C
        words = host_encode(np.stack([C, Fs], 1))
        if pairs is not None:
            assert [(int(c), int(f)) for c, f in zip(C, Fs)] == pairs
            assert [int(wd) for wd in words] == R.encode(pairs), n
        ideal = float((PB - np.log2(Fs.astype(np.float64))).sum())
        assert 32 * len(words) <= ideal + n / 64 + 64, (n, len(words), ideal)
        idx, state, err = host_decode(cums[np.arange(n) % 16], n, V, [words])
        assert idx[0].tolist() == syms and end_ok(state[0], err[0], len(words)), n
    if kind == 'least':
        assert ideal == 24.0 * 700
    toks, err, x, pos = R.decode([R.cumulative(tabs[i % 16]) for i in range(700)], [int(wd) for wd in words])
    assert toks == syms and (err, x, pos) == (0, R.LOW, len(words))      # codecref's own decoder reads the twin's stream


def test_state_carries_across_calls_and_images_are_independent():
    """two scales (l = 3, then l = 25) for three images with streams of different lengths, the state carried in `state`: the tokens of one
    call over all 28; V = 4096 takes the 64-entry segments of the search"""
    V = 4096
    tabs = _pool(V, 'random', seed=5)
    cum_all = np.array([R.cumulative(F) for F in tabs], np.uint32)
    n = 28
    syms, streams = [], []
    for b in range(3):
        s = _symbols(tabs, n, ['random', 'most', 'least'][b], 40 + b, shift=b)
        C = np.array([int(cum_all[(b + i) % 16][v - 1]) if v else 0 for i, v in enumerate(s)], np.int64)
        Fs = np.array([int(cum_all[(b + i) % 16][v]) for i, v in enumerate(s)], np.int64) - C
        syms.append(s); streams.append(host_encode(np.stack([C, Fs], 1)))
    assert len({len(s) for s in streams}) == 3
    rows = lambda lo, hi: np.concatenate([cum_all[(b + np.arange(lo, hi)) % 16] for b in range(3)])
    i0, state, err = host_decode(rows(0, 3), 3, V, streams)
    i1, state, err = host_decode(rows(3, n), n - 3, V, streams, state, err)
    for b in range(3):
        assert i0[b].tolist() + i1[b].tolist() == syms[b] and end_ok(state[b], err[b], len(streams[b]))


def test_corrupt_streams():
    """a truncated stream, one flipped word and an appended word each set err or fail the end check; the neighbours of a corrupt image are
    untouched; an image in error stays -1 in the next call"""
    V = 256
    tabs = _pool(V, 'random', seed=9)
    cums = np.array([R.cumulative(F) for F in tabs], np.uint32)
    n = 200
    syms = _symbols(tabs, n, 'random', 1)
    C = np.array([int(cums[i % 16][s - 1]) if s else 0 for i, s in enumerate(syms)], np.int64)
    Fs = np.array([int(cums[i % 16][s]) for i, s in enumerate(syms)], np.int64) - C
    words = host_encode(np.stack([C, Fs], 1))
    assert len(words) > 20
    flipped = words.copy(); flipped[10] ^= 0x00010000
    cum3 = np.concatenate([cums[np.arange(n) % 16]] * 3)
    for bad in (words[:-1], words[:1], words[:0], flipped, np.concatenate((words, [0x12345678])).astype(np.uint32)):
        idx, state, err = host_decode(cum3, n, V, [words, bad, words])
        assert idx[0].tolist() == syms and idx[2].tolist() == syms and end_ok(state[0], err[0], len(words)) and end_ok(state[2], err[2], len(words))
        assert not end_ok(state[1], err[1], len(bad))
        if err[1]:
            first = int(np.argmax(idx[1] == -1)) if (idx[1] == -1).any() else n
            assert (idx[1, first:] == -1).all() and (idx[1, :first] >= 0).all()
            idx2, _, err2 = host_decode(cum3, n, V, [words, bad, words], state.copy(), err.copy())
            assert (idx2[1] == -1).all() and err2[1] == err[1]
    idx, state, err = host_decode(cum3, n, V, [words, words[:-1], words])
    assert err[1] == 1 and idx[1, :100].tolist() == syms[:100]          # a truncated stream decodes until the missing word is asked for
    zero = np.zeros((n, V), np.uint32)                                  # a refused row's table: no slot has an owner
    idx, state, err = host_decode(zero, n, V, [words])
    assert err[0] == 2 and (idx == -1).all()


def test_refused_rows_and_invalid_tokens():
    B, l, V = 1, 4, 256
    logits = make_logits(B, l, V, seed=2)
    logits[0, 5] = np.nan
    logits[1, 6] = np.inf
    logits[2] = -np.inf
    gt = np.array([[3, 3, 3, V]], np.int64)
    cum, pairs, flags = host_table(logits, B, l, V, 0.0, None, gt)
    assert flags[0].tolist() == [1, 1, 1, 2] and not cum[:3].any() and not pairs.any() and cum[3, -1] == TOTAL
    logits = make_logits(B, l, V, seed=2)
    logits[B * l + 1, 9] = np.nan                                       # a NaN on the unconditional side reaches z as 0 * NaN
    _, _, flags = host_table(logits, B, l, V, 0.0)
    assert flags[0].tolist() == [0, 1, 0, 0]


def test_every_einval():
    from var_amd import abi
    B, l, V = 1, 2, 256
    logits = make_logits(B, l, V, seed=1)
    gt = np.zeros((B, l), np.int64)
    fn = _host('code_table_host_f32')
    cum, pairs, flags = np.zeros((B * l, V), np.uint32), np.zeros((B, l, 2), np.uint32), np.zeros((B, l), np.int32)
    P = lambda a: None if a is None else a.ctypes.data
    good = dict(logits=logits, B=B, l=l, V=V, gt=gt, ld=l, cum=cum, pairs=pairs, flags=flags)
    for change in (dict(logits=None), dict(flags=None), dict(cum=None, pairs=None, gt=None), dict(gt=None), dict(pairs=None), dict(B=0), dict(l=0),
                   dict(V=0), dict(V=255), dict(V=8448), dict(ld=l - 1)):
        a = {**good, **change}
        assert fn(P(a['logits']), a['B'], a['l'], a['V'], 0.0, None, P(a['gt']), a['ld'], P(a['cum']), P(a['pairs']), P(a['flags'])) == abi.EINVAL, change
    assert host_encode(np.array([[0, 0]]), expect=abi.EINVAL) is None                       # F == 0
    assert host_encode(np.array([[TOTAL - 1, 2]]), expect=abi.EINVAL) is None               # C + F > 2^PB
    assert host_encode(np.array([[0, 1]] * 8), cap=4, expect=abi.EINVAL) is None            # eight 24-bit symbols do not fit four words
    assert len(host_encode(np.zeros((0, 2)))) == 2                                            # no symbol: the state alone
    enc, dec = _host('rans_encode_host'), _host('rans_decode_host')
    w, nw = np.zeros(4, np.uint32), np.zeros(1, np.int64)
    assert enc(None, 0, P(w), 4, P(nw)) == abi.EINVAL and enc(P(w), -1, P(w), 4, P(nw)) == abi.EINVAL and enc(P(w), 0, P(w), 1, P(nw)) == abi.EINVAL
    off, st, idx, err = np.zeros(1, np.int64), np.zeros(4, np.uint32), np.zeros(l, np.int64), np.zeros(1, np.int32)
    args = [P(cum), l, V, P(w), 4, P(off), P(nw), P(st), P(idx), P(err), 1]
    assert dec(*args) == 0
    for pos, val in ((0, None), (3, None), (5, None), (6, None), (7, None), (8, None), (9, None), (1, 0), (2, 255), (2, 8448), (4, -1), (10, 0)):
        a = list(args); a[pos] = val
        assert dec(*a) == abi.EINVAL, (pos, val)
    nw[0] = 9                                                           # a word range outside `words`: err 3, nothing read
    st[:] = 0
    err[0] = 0
    assert dec(*args) == 0 and err[0] == 3 and (idx == -1).all()
