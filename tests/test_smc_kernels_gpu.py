"""The two kernels of VAR.sample_smc on the MI355X (include/var_hip.h).
varhip_smc_resample_f32: bit for bit against its host twin (itself pinned to the contract by tests/test_smc_resample_cpu.py) on the same cases,
every operand between guard bands.
varhip_kv_resample: byte for byte against numpy's gather applied to a copy, on tests/test_kv_compact_gpu.py's shapes; every cache lives between
guard bands built here (the entry point takes the caches through a host array of pointers) and every byte the contract does not name must keep
its value.  The refused rows (an out-of-range entry, a source that is no fixed point) are never dereferenced: nothing here provokes a fault."""
import numpy as np
import pytest
import torch

from tests import smcref as R
from tests import util
from tests.test_kv_compact_gpu import NP_DT
from var_amd import abi, hip

pytestmark = pytest.mark.gpu

CASES = R.cases()


def _twin(c):
    out = R.fresh_outputs(c)
    hip.call_host('smc_resample_host_f32', *R.call_args(c, out))
    return out


def _kernel(c, expect=0, seen=True):
    out = R.fresh_outputs(c, seen)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(v) for k, v in out.items()}
    args = R.call_args(dict(c, tokens=dev(c['tokens']), seeds=dev(c['seeds'])), d)
    if expect == 0:
        util.guarded_call('smc_resample_f32', *args)
    else:
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('smc_resample_f32', *args)
    return {k: None if v is None else v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize('c', CASES, ids=R.case_id)
def test_resample_kernel_equals_its_host_twin(c):
    got, want = _kernel(c), _twin(c)
    for k in R.FIELDS:
        assert R.same_bits(got[k], want[k]), (k, got[k], want[k])
    if c['ess_frac'] < 0 and c['n'] > 1 and c['beta'] == 50:
        assert (got['anc'] != np.tile(np.arange(c['n']), c['images'])).any(), 'no slot was overwritten: the case shows nothing'


def test_resample_kernel_edge_weights_and_null_seen():
    def weights(logw, images=1):
        logw = np.asarray(logw, np.float64)
        return dict(tokens=None, ld_img=0, ld_cls=0, images=images, n=logw.size // images, t0=0, t1=0, beta=1.0, logw=logw.reshape(-1),
                    seeds=np.arange(images, dtype=np.int64) + 5, scale=3, ess_frac=-1.0)
    dominant = np.full(8, -2.0); dominant[3] = 1000.0
    for logw, images in (([0.5, np.nan, 0.1, -0.3, np.nan, 0.0, 0.2, -1.0], 1), ([np.nan] * 4, 1), ([-np.inf] * 4, 1), ([0.0, np.inf, 1.0, np.nan], 1),
                         ([np.nan, np.nan, np.nan, 0.0, 5.0, 1.0], 2), ([0.3] * 8, 1), (dominant, 1), (np.linspace(-3, 0, 2048), 1)):
        c = weights(logw, images)
        got, want = _kernel(c), _twin(c)
        for k in R.FIELDS:
            assert R.same_bits(got[k], want[k]), (k, logw)
    c = R.make_case(8, 1, -1)
    got, want = _kernel(c, seen=False), _twin(c)
    for k in ('anc', 'did', 'ess', 'logw'):
        assert R.same_bits(got[k], want[k]), k


def test_resample_kernel_einval_writes_nothing():
    c = R.make_case(8, 1, -1)
    for kw in (dict(n=0), dict(n=2049), dict(images=0), dict(t0=-1), dict(t1=c['t0'] - 1), dict(scale=-1), dict(ld_cls=c['t1'] - 1),
               dict(ld_img=8 * c['ld_cls'] - 1), dict(tokens=None), dict(seeds=None)):
        got = _kernel(dict(c, **kw), expect=abi.EINVAL)
        fresh = R.fresh_outputs(dict(c, **kw))
        for k in R.FIELDS:
            assert R.same_bits(got[k], fresh[k]), (kw, k)
    for k in ('logw', 'anc', 'did', 'ess'):                  # a NULL output
        out = {f: torch.from_numpy(v).cuda() for f, v in R.fresh_outputs(c).items()}
        out[k] = None
        dev = dict(c, tokens=torch.from_numpy(c['tokens']).cuda(), seeds=torch.from_numpy(c['seeds']).cuda())
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('smc_resample_f32', *R.call_args(dev, out))


# ---- varhip_kv_resample ---------------------------------------------------------------------------------------------------------------------
ROWS = 8
TABLES = {
    'identity': [0, 1, 2, 3, 4, 5, 6, 7],
    'one_dead': [0, 1, 2, 5, 4, 5, 6, 7],
    'all_but_one_dead': [6, 6, 6, 6, 6, 6, 6, 6],
    'cond_uncond': [0, 0, 2, 2, 4, 4, 6, 6],                 # step (b): R = 4 rows [0, 0, 2, 2] and the same table shifted by R behind it
}


def _caches(nbuf, H, Lmax, esz, rows=ROWS):
    """[buffer][row][head][token][channel] integers that encode their own position (16-bit caches: modulo the prime 65521)"""
    b, r, h, t, c = np.meshgrid(np.arange(nbuf), np.arange(rows), np.arange(H), np.arange(Lmax), np.arange(64), indexing='ij')
    code = ((((b * rows + r) * H + h) * Lmax + t) * 64 + c + 1).astype(np.int64)
    return (code if esz == 4 else code % 65521).astype(NP_DT[esz])


def _want(buf_np, idx, ln):
    """numpy's gather applied to a copy; rows the kernel must refuse keep their bytes"""
    idx = np.asarray(idx)
    want, bad = buf_np.copy(), 0
    for r, s in enumerate(idx):
        if s == r:
            continue
        if not 0 <= s < len(idx) or idx[s] != s:
            bad += 1
            continue
        want[:, r, :, :ln] = buf_np[:, s, :, :ln]
    return want, bad


def _run(buf_np, idx, H, Lmax, ln, esz, expect_rc=0, ptrs=None, rows=None, nbuf_arg=None, null=None):
    nbuf = buf_np.shape[0]
    bufs = [torch.from_numpy(buf_np[i].view(np.uint8).copy()).cuda() for i in range(nbuf)]
    arenas, placed = util.guard_layout(bufs)
    assert len(arenas) == nbuf
    ptr = {pos: ar.ptr(addr) for pos, addr, _, ar in placed}
    bp = torch.tensor([ptr[i] for i in range(nbuf)] if ptrs is None else ptrs(ptr), dtype=torch.int64)
    idx_d = torch.tensor(idx, dtype=torch.int32, device='cuda')
    bad = torch.zeros(1, dtype=torch.int32, device='cuda')
    args = [bp, len(bp), idx_d, len(idx) if rows is None else rows, H, Lmax, ln, esz, bad]
    if nbuf_arg is not None:
        args[1] = nbuf_arg
    if null is not None:                                     # a NULL in place of the pointer table, the index table or the counter
        args[dict(bufs=0, idx=2, bad=8)[null]] = None
    if expect_rc == 0:
        util.guarded_call('kv_resample', *args)
    else:
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('kv_resample', *args)
    torch.cuda.synchronize()
    found = [f for ar in arenas for f in ar.findings('varhip_kv_resample')]
    assert not found, found
    for pos, addr, b, ar in placed:
        ar.get(addr, b)
    return np.stack([t.cpu().numpy().view(buf_np.dtype).reshape(buf_np.shape[1:]) for t in bufs]), int(bad.item())


@pytest.mark.parametrize('esz', [4, 2])
@pytest.mark.parametrize('H, Lmax, mid', [(2, 14, 5), (16, 55, 30), (16, 14, 5), (2, 55, 30)])
def test_rows_that_died_take_their_ancestors_bytes_and_nothing_else_changes(H, Lmax, mid, esz):
    """len in {1, a scale end (patch_nums 1 2 3: 5 of 14; 1 2 3 4 5: 30 of 55), Lmax}; 2 and 6 buffers; the four tables of a call"""
    for blocks in (1, 3):
        buf_np = _caches(2 * blocks, H, Lmax, esz)
        for ln in (1, mid, Lmax):
            for kind, idx in TABLES.items():
                want, nbad = _want(buf_np, idx, ln)
                got, bad = _run(buf_np, idx, H, Lmax, ln, esz)
                assert nbad == 0 and bad == 0 and np.array_equal(got, want), (blocks, ln, kind)
                assert (kind == 'identity') == np.array_equal(got, buf_np)


def test_whole_tiles_and_a_partial_last_tile():
    """H * len * 16 vectors per row = 1024 * 2 + 384 at H = 19, len = 8, fp32: two whole 1024-vector tiles and a partial one per (buffer, row)"""
    H, Lmax, ln, esz = 19, 9, 8, 4
    buf_np = _caches(2, H, Lmax, esz)
    for kind in ('one_dead', 'all_but_one_dead', 'cond_uncond'):
        want, _ = _want(buf_np, TABLES[kind], ln)
        got, bad = _run(buf_np, TABLES[kind], H, Lmax, ln, esz)
        assert bad == 0 and np.array_equal(got, want) and not np.array_equal(got, buf_np), kind


@pytest.mark.parametrize('idx, nbad', [([1, 2, 2, 3, 4, 5, 6, 7], 1),          # row 0's source, row 1, is itself overwritten: not a fixed point
                                       ([3, 3, 2, 1, 4, 5, 6, 7], 3),          # a cycle through rows 0, 1 and 3 (none is a fixed point); row 2 stays
                                       ([8, 1, -1, 3, 2 ** 31 - 1, 5, 7, 7], 3),   # out of range on both sides; row 6 still takes row 7
                                       ([0, 1, 2, 3, 4, 5, 6, 0], 0)])
def test_refused_rows_stay_unwritten_and_are_counted_once(idx, nbad):
    H, Lmax, ln = 16, 14, 14                                 # 14 tiles' worth of vectors per (buffer, row) over 6 buffers: many workgroups see each refused row
    for esz in (4, 2):
        buf_np = _caches(6, H, Lmax, esz)
        want, n = _want(buf_np, idx, ln)
        got, bad = _run(buf_np, idx, H, Lmax, ln, esz)
        assert n == nbad and bad == nbad and np.array_equal(got, want), (idx, esz, bad)


def test_einval_writes_nothing_and_empty_calls_succeed():
    H, Lmax, esz = 2, 14, 4
    buf_np = _caches(2, H, Lmax, esz)
    idx = TABLES['one_dead']
    nbytes = ROWS * H * Lmax * 64 * esz
    bad_calls = [dict(ln=Lmax + 1), dict(ln=-1), dict(esz=1), dict(esz=8), dict(esz=3), dict(rows=-1), dict(H=0), dict(Lmax=0), dict(nbuf_arg=0),
                 dict(null='bad'), dict(null='idx'), dict(null='bufs'),
                 dict(ptrs=lambda p: [p[0], p[0]]),                              # the same cache twice
                 dict(ptrs=lambda p: [p[0], p[0] + nbytes - 16]),                # the second starts in the first's last vector
                 dict(ptrs=lambda p: [p[0], p[1] + 8]),                          # a misaligned pointer
                 dict(ptrs=lambda p: [p[0], 0])]                                 # a NULL cache
    for kw in bad_calls:
        a = dict(H=H, Lmax=Lmax, ln=5, esz=esz)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        got, bad = _run(buf_np, idx, a['H'], a['Lmax'], a['ln'], a['esz'], expect_rc=abi.EINVAL, **kw)
        assert bad == 0 and np.array_equal(got, buf_np), kw
    for kw in (dict(ln=0), dict(ln=5, rows=0)):
        got, bad = _run(buf_np, idx, H, Lmax, kw['ln'], esz, rows=kw.get('rows'))
        assert bad == 0 and np.array_equal(got, buf_np), kw
