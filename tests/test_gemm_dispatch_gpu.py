"""Every path varhip_gemm_nt_f32 and varhip_gemm_qkv_f32 can dispatch to (var_amd/csrc/gemm.hip: four DMA tiles, the k_gemm_any fallback,
the three epilogues of each tile (the lean one of full tiles, the general loop with 16-byte accesses, the general loop element by element),
k_gemm_any's own epilogue, the two gemm_qkv tiles), on every operand geometry that selects among them.

The cases, the NaN-padded operands, the sentinel-filled outputs and the float64 bound are tests/gemmcases.py (validated on the twins alone
by tests/test_gemm_dispatch_cpu.py).  Here every call goes through both(): guard bands on both sides, the HIP result bit for bit equal to
the oracle's INCLUDING the untouched padding of `out`, varhip_gemm_last_pick() equal to the path the case was built for (the tile forced
with varhip_gemm_force_tile, or 3 = k_gemm_any where the fast path's conditions do not hold), varhip_gemm_last_evec() equal to the epilogue
switch the case was built for (a 16-byte access at a 4-byte aligned address gives the same bits, so results cannot show a missing term of that
predicate; the hook does), and the float64 bound on top — the oracle
is a twin written beside the kernel, float64 numpy is not."""
import numpy as np
import pytest

from tests import gemmcases as gc
from tests import util
from tests.test_kernels_gpu import _setup, both
from var_amd import abi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def hooks_reset():
    yield
    _, hip = _setup()
    so = hip.lib().so
    so.varhip_gemm_force_tile(-1); so.varhip_gemm_qkv_force_tile(-1); so.varhip_gemm16_force_tile(-1); so.varhip_gemm16_deep(1)


def gpu_call(c, name, args, outs):
    """call(...) of gemmcases.run_case: force the case's tile, run both libraries, compare bit for bit, check the reported path"""
    _, hip = _setup()
    so = hip.lib().so
    hook = so.varhip_gemm_force_tile if name == 'gemm_nt_f32' else so.varhip_gemm_qkv_force_tile
    hook(c['tile'])
    try:
        got, want = both(name, args, outs)
        pick, evec = so.varhip_gemm_last_pick(), so.varhip_gemm_last_evec()
    finally:
        hook(-1)
    for g, w in zip(got, want):
        gb, wb = gc.bits(g).reshape(-1), gc.bits(w).reshape(-1)
        bad = np.flatnonzero(gb != wb)
        assert bad.size == 0, (f"{c['name']}: {bad.size}/{gb.size} elements differ from the oracle bit for bit, first at flat element {int(bad[0])}: "
                               f"got {g.reshape(-1)[bad[0]]!r} want {w.reshape(-1)[bad[0]]!r}")
    if c['pick'] is not None:
        assert pick == c['pick'], f"{c['name']}: dispatched to path {pick}, expected {c['pick']}"
    if c.get('evec') is not None:
        assert evec == c['evec'], f"{c['name']}: varhip_gemm_last_evec() = {evec}, expected {c['evec']}"
    return got


def _run(cases):
    for c in cases:
        gc.run_case(c, gpu_call)


@pytest.mark.parametrize('tile', [0, 1, 2, 3])
def test_every_tile_on_ragged_shapes(tile):
    """12 seeded (M, N, K) triples over M in {1, 31, 33, 65, 129, 130}, N in {4, 36, 68, 132, 260}, K in {32, 256, 288} and all three epilogues on
    the forced tile (last_pick: 0, 1, 2 and 4 for the hook's tile 3), bias / gamma NULL on some, rows_per_group = 7; and one forced call with
    K = 40, which must still take the fallback (last_pick 3)"""
    _run([c for c in gc.ragged_cases() if c['tile'] == tile])


def test_every_vec_condition_alone():
    """lda, ldw, the alignment of A (offsets 1, 2, 3) and W, sA, sW, K % 32: each alone sends the call to k_gemm_any (last_pick 3); the padded
    controls (lda + 4, ldw + 8, A + 4, sA + 4, sW + 4) stay on the forced tile 2"""
    _run(gc.vec_cases())


@pytest.mark.parametrize('tile', [0, 1, 2, 3])
def test_every_evec_condition_alone(tile):
    """N % 4, ldo, out, bias, ldr, resid, ldg, gamma, sO: each alone turns the 16-byte epilogue accesses off (last_evec 0); the padded controls
    (ldo + 4, ldr + 8, ldg = 2N with gamma at N, all of them with interior pointers, sO + 4) keep them (1); the call stays on the forced tile"""
    _run([c for c in gc.evec_cases() if c['tile'] == tile])


def test_fallback_on_padded_geometry():
    """k_gemm_any's own epilogue: ldo, ldr, ldg padded by multiples of 4 and by odd amounts, gamma at an interior pointer, every pointer
    misaligned at once, a padded batch stride, at K = 40 (last_pick 3, last_evec -1)"""
    _run(gc.fallback_cases())


@pytest.mark.parametrize('tile', [0, 1, 2, 3, None])
def test_batched(tile):
    _run([c for c in gc.batched_cases() if (c['pick'] == gc.PICK_ANY) == (tile is None) and (tile is None or c['tile'] == tile)])


def test_batched_resid_or_gamma_is_refused():
    """VARHIP_EINVAL from both libraries, `out` left at the sentinel, no band touched"""
    _, hip = _setup()
    L, _ = _setup()
    for c in gc.einval_cases():
        b = gc.build(c)
        dev = {}
        def d(a):
            if isinstance(a, tuple):
                return d(a[0])[a[1]:]
            if isinstance(a, np.ndarray):
                if id(a) not in dev:
                    dev[id(a)] = torch.from_numpy(a).cuda()
                return dev[id(a)]
            return a
        args = [d(a) for a in b.args]
        rc = util.guarded_invoke('varhip_gemm_nt_f32', args, lambda *a: hip.lib().fn['gemm_nt_f32'](*a, hip.current_stream()), torch.cuda.synchronize)
        assert rc == abi.EINVAL, f"{c['name']}: rc={rc}"
        gc.verify_nt(b, dev[id(b.out)].cpu().numpy())
        gc.run_case(c, gc.host_call(L))


@pytest.mark.parametrize('HW', [36, 100])
def test_attnblock_geometry_at_ragged_size(HW):
    """the four products of the VAE AttnBlock (var_amd/engine.py attnblock: interior weight / bias pointers, bias per row, lda = ldw = 2 Cc with
    W = qk + Cc, batch strides) at Cc = 32 and HW = 36 / 100, on the automatic pick and on every forced tile; p . v has K = HW: the fallback"""
    for tile in (-1, 0, 1, 2, 3):
        gc.attn_chain(gpu_call, Cc=32, HW=HW, tile=tile)


@pytest.mark.parametrize('tile', [0, 1])
def test_gemm_qkv_both_tiles(tile):
    _run([c for c in gc.qkv_cases() if c['tile'] == tile])


def test_gemm_qkv_rejections_leave_outputs_untouched():
    """K % 32, lda % 4, ldw % 4, each of the six pointers misaligned, C != 64 H, M != B2 l, pos0 + l > Lmax: VARHIP_EINVAL, q_out and the caches
    still the sentinel, no band touched"""
    _, hip = _setup()
    base = gc.qkv('qkv reject', 4, 9, 2, 128, 5, 14, 1)
    bad = [('K%32', {7: 96 + 8}), ('lda%4', {1: 130}), ('ldw%4', {3: 130}), ('A+1', {0: 1}), ('W+1', {2: 1}), ('bias+1', {4: 1}), ('q_out+1', {11: 1}),
           ('kcache+1', {12: 1}), ('vcache+1', {13: 1}), ('C!=64H', {6: 192}), ('M!=B2*l', {5: 35}), ('pos0+l>Lmax', {17: 6})]
    for nm, change in bad:
        b = gc.build(base)
        ten = {}
        args = []
        for i, a in enumerate(b.args):
            if isinstance(a, np.ndarray):
                t = ten.setdefault(i, torch.from_numpy(np.concatenate([a.reshape(-1), gc.sentinel(4)])).cuda())      # (room for the shifted pointers)
                args.append(t[change[i]:] if i in change else t[:a.size])
            else:
                args.append(change.get(i, a))
        rc = util.guarded_invoke('varhip_gemm_qkv_f32', args, lambda *a: hip.lib().fn['gemm_qkv_f32'](*a, hip.current_stream()), torch.cuda.synchronize)
        assert rc == abi.EINVAL, f'{nm}: rc={rc}'
        for i in (11, 12, 13):
            assert bool((gc.bits(ten[i].cpu().numpy()) == gc.SENTINEL_BITS).all()), f'{nm}: a refused call wrote to argument {i}'


D16_SHAPES = [(2 * 64 * l, N, K, epi) for l in (1, 4, 9, 256)
              for N, K, epi in ((1024, 1024, abi.EPI_RESID), (4096, 1024, abi.EPI_GELU), (1024, 4096, abi.EPI_RESID), (4096, 1024, abi.EPI_NONE),
                                (3072, 1024, abi.EPI_NONE))]       # proj, fc1, fc2, head, mat_qkv's shape at B = 64, d16 (C = 1024)


def test_automatic_picker_reaches_every_tile():
    """no forcing, the d16 production shapes M = 2 B l (B = 64, l in {1, 4, 9, 256}) x the layer shapes over 1024 / 3072 / 4096: each of the four
    DMA tiles (last_pick 0, 1, 2, 4) must be the cost model's choice for at least one of them — a tile no production shape reaches is dead
    code or a shifted cost model"""
    _, hip = _setup()
    fn, so = hip.lib().fn, hip.lib().so
    so.varhip_gemm_force_tile(-1)
    picks = {}
    A = torch.zeros(32768 * 4096, device='cuda'); W = torch.zeros(4096 * 4096, device='cuda'); out = torch.empty(32768 * 4096, device='cuda')
    bias = torch.zeros(4096, device='cuda'); gamma = torch.zeros(128 * 4096, device='cuda')
    for M, N, K, epi in D16_SHAPES:
        res = epi == abi.EPI_RESID
        hip.call('gemm_nt_f32', A, K, W, K, bias, out, N, M, N, K, epi, A if res else None, N, gamma if res else None, N, M // 128, 0, 1, 0, 0, 0)
        picks[(M, N, K, epi)] = so.varhip_gemm_last_pick()
    torch.cuda.synchronize()
    print(picks)
    for tile in (0, 1, 2, 4):
        assert tile in picks.values(), f'path {tile} is the automatic pick of none of the d16 shapes (M, N, K, epi) -> pick: {picks}'
    assert gc.PICK_ANY not in picks.values()


@pytest.mark.parametrize('tile', [0, 1, 2, 3])
@pytest.mark.parametrize('flavour', ['f16', 'bf16'])
def test_gemm16_padded_geometry_every_tile(flavour, tile):
    """the 16-bit GEMM on padded operands: lda = K + 8, ldw = K + 16, ldo = N + 4, ldr = N + 4, interior pointers at 16-byte multiples, NaN padding,
    sentinel-filled out; against float64 on the 16-bit inputs with test_gemm16_against_float64's tolerance (gemmcases.gemm16_tolerance)"""
    _, hip = _setup()
    dt, ulp = (torch.float16, 2.0 ** -10) if flavour == 'f16' else (torch.bfloat16, 2.0 ** -7)      # (the 16-bit rounding term of tests/test_f16_gpu.py / test_bf16_gpu.py)
    sent16 = torch.tensor([0x7E5A if flavour == 'f16' else 0x7FE5], dtype=torch.int16).view(dt)
    sent32 = torch.from_numpy(gc.sentinel(1))
    for M, N, K in ((130, 132, 128), (33, 260, 64)):
        for mode in ('none16', 'resid32'):
            g = torch.Generator().manual_seed(M + N + tile)
            out16 = mode == 'none16'
            def alloc(off, rows, ld, cols, scale, dtype):
                flat = torch.full((off + (rows - 1) * ld + cols + gc.TAIL,), float('nan'), dtype=dtype)
                real = (torch.randn(rows, cols, generator=g) * scale).to(dtype)
                flat[off:off + (rows - 1) * ld + cols].as_strided((rows, cols), (ld, 1)).copy_(real)
                return flat, real.double()
            lda, ldw, ldo, ldr, rpg = K + 8, K + 16, N + 4, N + 4, 50
            G = (M + rpg - 1) // rpg
            A, A64 = alloc(8, M, lda, K, 0.7, dt); W, W64 = alloc(16, N, ldw, K, 1.5 / K ** 0.5, dt)
            bias, b64 = alloc(4, 1, N, N, 0.2, torch.float32); resid, r64 = alloc(4, M, ldr, N, 1.0, torch.float32)
            gamma, g64 = alloc(4, G, N + 4, N, 0.5, torch.float32)
            ooff = 8 if out16 else 4
            n_out = ooff + (M - 1) * ldo + N + gc.TAIL
            out = (sent16 if out16 else sent32).repeat(n_out)
            inside = torch.zeros(n_out, dtype=torch.bool)
            inside[ooff:ooff + (M - 1) * ldo + N].as_strided((M, N), (ldo, 1)).fill_(True)
            epi = abi.EPI_RESID if mode == 'resid32' else abi.EPI_NONE
            dA, dW, dB, dR, dG, dO = (t.cuda() for t in (A, W, bias, resid, gamma, out))
            hip.lib().so.varhip_gemm16_force_tile(tile)
            try:
                util.guarded_call(f'gemm_nt_{flavour}', dA[8:], lda, dW[16:], ldw, dB[4:], dO[ooff:], ldo, int(out16), M, N, K, epi,
                                  dR[4:] if epi else None, ldr, 0, dG[4:] if epi else None, N + 4, rpg, 1, 0, 0, 0)
            finally:
                hip.lib().so.varhip_gemm16_force_tile(-1)
            res = dO.cpu()
            raw, sraw = (res.view(torch.int16), out.view(torch.int16)) if out16 else (res.view(torch.int32), out.view(torch.int32))
            name = f'gemm16 {flavour} t{tile} {M}x{N}x{K} {mode}'
            assert bool((raw[~inside] == sraw[~inside]).all()), f'{name}: padding of out was written'
            assert not bool((raw[inside] == sraw[inside]).any()), f'{name}: elements inside [M][N] were not written'
            got = res[ooff:ooff + (M - 1) * ldo + N].as_strided((M, N), (ldo, 1)).double()
            assert bool(torch.isfinite(got).all()), f'{name}: non-finite results (a padding element was read?)'
            ref = A64 @ W64.T + b64
            mag = A64.abs() @ W64.abs().T
            gabs = None
            if epi:
                gm = g64.repeat_interleave(rpg, dim=0)[:M]
                ref = r64 + ref * gm; gabs = gm.abs().numpy()
            tol = gc.gemm16_tolerance(mag.numpy(), ref.numpy(), out16, gabs, ulp16=ulp)
            err = (got - ref).abs().numpy()
            assert bool((err <= tol).all()), f'{name}: {int((err > tol).sum())} outside tolerance, max err {float(err.max()):.3e}'
