"""varhip_kv_compact on the MI355X (include/var_hip.h): the row gather of the per-block KV caches, byte for byte against numpy's
gather.  Every cache lives between guard bands (tests.util: the bands of the caches are built here, since the entry point takes them through
host arrays of pointers; idx and the pointer arrays go through guarded_call), the destination is pre-filled with a sentinel pattern, and
everything the contract does not name — tokens >= len, rows >= rows_out, the sources, the bands — must keep its bytes."""
import numpy as np
import pytest
import torch

from tests import util
from var_amd import hip

pytestmark = pytest.mark.gpu

ROWS_SRC, ROWS_DST, ROWS_OUT = 6, 4, 3
SENTINEL = 0xA5
IDX = {'duplicate': [4, 1, 4], 'descending': [5, 2, 3], 'identity': [0, 1, 2]}
NP_DT = {4: np.uint32, 2: np.uint16}


def _source(nbuf, H, Lmax, esz):
    """[buffer][row][head][token][channel] integers that encode their own position (buffer = 2 * block + k-or-v); 16-bit caches hold them modulo
    65521 (a prime: neighbours in every dimension still differ)"""
    b, r, h, t, c = np.meshgrid(np.arange(nbuf), np.arange(ROWS_SRC), np.arange(H), np.arange(Lmax), np.arange(64), indexing='ij')
    code = ((((b * ROWS_SRC + r) * H + h) * Lmax + t) * 64 + c + 1).astype(np.int64)
    return (code if esz == 4 else code % 65521).astype(NP_DT[esz])


def _run(src_np, dst_np, idx, rows_out, H, Lmax, ln, esz, expect_rc=0, rows_dst=None, dst_ptrs=None):
    """the call on device copies of src_np / dst_np [buffer][rows]... inside guard arenas -> (src after, dst after) as numpy arrays"""
    nbuf = src_np.shape[0]
    src = [torch.from_numpy(src_np[i].view(np.uint8).copy()).cuda() for i in range(nbuf)]
    dst = [torch.from_numpy(dst_np[i].view(np.uint8).copy()).cuda() for i in range(nbuf)]
    arenas, placed = util.guard_layout(src + dst)
    assert len(arenas) == 2 * nbuf
    ptr = {pos: ar.ptr(addr) for pos, addr, _, ar in placed}
    sp = torch.tensor([ptr[i] for i in range(nbuf)], dtype=torch.int64)
    dp = torch.tensor([ptr[nbuf + i] for i in range(nbuf)] if dst_ptrs is None else dst_ptrs(ptr), dtype=torch.int64)
    idx_d = torch.tensor(idx, dtype=torch.int32, device='cuda')
    args = (sp, dp, nbuf, idx_d, ROWS_SRC, ROWS_DST if rows_dst is None else rows_dst, rows_out, H, Lmax, ln, esz)
    if expect_rc == 0:
        util.guarded_call('kv_compact', *args)
    else:
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('kv_compact', *args)
    torch.cuda.synchronize()
    found = [f for ar in arenas for f in ar.findings('varhip_kv_compact')]
    assert not found, found
    for pos, addr, b, ar in placed:
        ar.get(addr, b)
    back = lambda ts, like: np.stack([t.cpu().numpy().view(like.dtype).reshape(like.shape[1:]) for t in ts])
    return back(src, src_np), back(dst, dst_np)


def _sentinel(nbuf, H, Lmax, esz, rows=ROWS_DST):
    return np.full((nbuf, rows, H, Lmax, 64), SENTINEL * (0x01010101 if esz == 4 else 0x0101), dtype=NP_DT[esz])


@pytest.mark.parametrize('esz', [4, 2])
@pytest.mark.parametrize('H, Lmax, mid', [(2, 14, 5), (16, 55, 30), (16, 14, 5), (2, 55, 30)])
def test_gather_is_numpys_and_nothing_else_is_written(H, Lmax, mid, esz):
    """len in {1, a scale boundary in the middle (patch_nums 1 2 3: 5 of 14; 1 2 3 4 5: 30 of 55), Lmax}; 1 and 3 blocks (2 and 6 buffers); idx
    with a duplicate, a descending pair and the identity"""
    for blocks in (1, 3):
        nbuf = 2 * blocks
        src_np = _source(nbuf, H, Lmax, esz)
        for ln in (1, mid, Lmax):
            for kind, idx in IDX.items():
                dst_np = _sentinel(nbuf, H, Lmax, esz)
                want = dst_np.copy()
                want[:, :ROWS_OUT, :, :ln] = src_np[:, idx][:, :, :, :ln]
                src_after, got = _run(src_np, dst_np, idx, ROWS_OUT, H, Lmax, ln, esz)
                assert np.array_equal(got, want), (blocks, ln, kind)
                assert np.array_equal(src_after, src_np), (blocks, ln, kind)


def test_rows_that_fill_whole_tiles_and_a_partial_last_tile():
    """H * len * 16 vectors per row = 1024 * 2 + 384 at H = 19, len = 8, fp32: two whole 1024-vector tiles and a partial one per (buffer, row)"""
    H, Lmax, ln, esz = 19, 9, 8, 4
    src_np = _source(2, H, Lmax, esz)
    dst_np = _sentinel(2, H, Lmax, esz)
    want = dst_np.copy()
    want[:, :ROWS_OUT, :, :ln] = src_np[:, IDX['duplicate']][:, :, :, :ln]
    src_after, got = _run(src_np, dst_np, IDX['duplicate'], ROWS_OUT, H, Lmax, ln, esz)
    assert np.array_equal(got, want) and np.array_equal(src_after, src_np)


def test_a_source_row_out_of_range_leaves_its_destination_row_alone():
    H, Lmax, esz = 2, 14, 4
    src_np, dst_np = _source(2, H, Lmax, esz), _sentinel(2, H, Lmax, esz)
    want = dst_np.copy()
    want[:, 1, :, :5] = src_np[:, 3, :, :5]
    _, got = _run(src_np, dst_np, [ROWS_SRC, 3, -1], ROWS_OUT, H, Lmax, 5, esz)
    assert np.array_equal(got, want)


def test_einval_writes_nothing_and_empty_calls_succeed():
    H, Lmax, esz = 2, 14, 4
    src_np = _source(2, H, Lmax, esz)
    idx = IDX['identity']
    bad = [dict(ln=Lmax + 1), dict(ln=-1), dict(rows_out=ROWS_DST + 1), dict(esz=1), dict(esz=8), dict(esz=3),
           dict(dst_ptrs=lambda p: [p[2], p[0] + 64]),                          # the second destination starts inside the first source
           dict(dst_ptrs=lambda p: [p[2], p[1] - ROWS_DST * H * Lmax * 64 * esz + 16])]   # ... ends 16 bytes inside the second source
    for kw in bad:
        dst_np = _sentinel(2, H, Lmax, esz)
        a = dict(rows_out=ROWS_OUT, ln=5, esz=esz, dst_ptrs=None)
        a.update(kw)
        src_after, got = _run(src_np, dst_np, idx + [0, 0], a['rows_out'], H, Lmax, a['ln'], a['esz'], expect_rc=-1, dst_ptrs=a['dst_ptrs'])
        assert np.array_equal(got, dst_np) and np.array_equal(src_after, src_np), kw
    for kw in (dict(ln=0, rows_out=ROWS_OUT), dict(ln=5, rows_out=0)):
        dst_np = _sentinel(2, H, Lmax, esz)
        src_after, got = _run(src_np, dst_np, idx, kw['rows_out'], H, Lmax, kw['ln'], esz)
        assert np.array_equal(got, dst_np) and np.array_equal(src_after, src_np), kw
