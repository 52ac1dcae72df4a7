"""One case table, one operand builder and one float64 reference for the 16-bit GEMMs of var_amd/csrc/gemm16.hip (varhip_gemm_nt_* and
varhip_gemm_qkv_*), shared by tests/test_gemm16_dispatch_cpu.py (the table against a restatement of the dispatch, the conditions on the
reference and the planted faults, no GPU) and tests/test_gemm16_dispatch_gpu.py (every instantiation on the GPU).

Cases.  A case names the entry point ('nt', 'qkv'), the shape, the paddings of the leading dimensions, the epilogue, the store and residual
types, rows_per_group, batch and the slack of the batch strides, the forced tile (-1: the automatic picker), the persistence and deep
switches, and `expect` = (varhip_gemm16_last_pick(0), varhip_gemm16_last_pick(1)) after the call (include/var_hip.h:
TMW * 1000 + TNW * 100 + WN * 10 + NST, 8440 for k_gemm16p, 0 for a launch the call does not make).  `expect` is written down per group of
the table from the kernel the group is built for; tests/test_gemm16_dispatch_cpu.py restates the dispatch on its own and compares.

Exact cases (epilogues NONE and RESID, q/k/v with l2norm = 0).  A holds integers in [-2, 2]; W integers in [-2, 2] times 2^-s for even k
and 2^-(s + 8) for odd k; the bias fp32 multiples of 2^-10 in [-2, 2]; a 16-bit residual multiples of 2^-4 in [-4, 4] (exact in fp16 and in
bfloat16); gamma +-2^e times 1 or 3, e in -2 .. 1, drawn per (row group, column), so any two row groups differ in 15 of 16 columns; the
q scale of l2norm = 0 is 2^-3.  Every product and every partial sum, in ANY order, is a multiple of the finest grid in use and stays below
2^24 units of it (exactness_budget, asserted per case): exact in fp32.  Whatever tile, pipeline depth or launch split ran, a correct kernel
holds the exact value and rounds it ONCE; the expectation is float64 arithmetic cast once, compared bit for bit on NaN-filled buffers
(padding of `out`, cache rows outside [pos0, pos0 + l) must still hold the fill).  s puts the deviation of the coarse half of the K sum
near 8 (shift_of), so with the fine half and the bias the exact value needs up to 15 bits: the sum before the bias, the sum before the
residual and the final value each need a real rounding (tests/test_gemm16_dispatch_cpu.py asserts the shares).

An fp32 residual lies on multiples of 2^-12 in [-4, 4], NOT on the 2^-4 grid of the 16-bit one: every multiple of 2^-4 in [-4, 4] fits the
8 bits of bfloat16, so on that grid a kernel reading the fp32 residual through 16 bits would compute the same bits and the planted fault
'resid_through_16' could change no expectation.  The budget covers the finer grid.

GELU and l2norm = 1 cannot be dyadic.  They use normal operands, the bars of the existing tests against float64 (gemm16_tolerance of
tests/gemmcases.py; one 16-bit rounding + 2e-4 for q/k/v), and must be bit-equal across every instantiation that can run the same call
(equal_groups)."""
import math
import zlib

import torch

FLAVOURS = ('f16', 'bf16')
DTYPE = {'f16': torch.float16, 'bf16': torch.bfloat16}
ULP16 = {'f16': 2.0 ** -10, 'bf16': 2.0 ** -7}      # the 16-bit rounding term of tests/test_f16_gpu.py / tests/test_bf16_gpu.py
NAN = float('nan')
FINE = 8                                             # odd k: weights on a grid 2^-FINE finer than even k
BIAS_GRID, RES16_GRID, RES32_GRID = 2.0 ** -10, 2.0 ** -4, 2.0 ** -12
Q_PLAIN = 0.125
# varhip_gemm16_last_pick codes
K128, K32D, K64D, K64, K192, K256, KP = 4422, 1124, 2224, 2222, 6442, 8442, 8440
Q32D, Q64D, Q64 = 1423, 2423, 2422
# how a forced call reaches an instantiation, its tile and its LDS stages (k_gemm16p: two stages)
NT_INST = {K128: dict(tile=0, persist=1, deep=1, bm=128, bn=128, nst=2), K32D: dict(tile=1, persist=1, deep=1, bm=32, bn=32, nst=4),
           K64D: dict(tile=1, persist=1, deep=1, bm=64, bn=64, nst=4), K64: dict(tile=1, persist=1, deep=0, bm=64, bn=64, nst=2),
           K192: dict(tile=3, persist=1, deep=1, bm=192, bn=256, nst=2), K256: dict(tile=2, persist=0, deep=1, bm=256, bn=256, nst=2),
           KP: dict(tile=2, persist=1, deep=1, bm=256, bn=256, nst=2)}
QKV_INST = {Q32D: dict(tile=1, persist=1, deep=1, bm=32, bn=128, nst=3), Q64D: dict(tile=1, persist=1, deep=1, bm=64, bn=128, nst=3),
            Q64: dict(tile=1, persist=1, deep=0, bm=64, bn=128, nst=2), K128: NT_INST[K128], K192: NT_INST[K192], K256: NT_INST[K256], KP: NT_INST[KP]}
FILL_K = {2: (64, 128, 192), 3: (64, 128, 192, 256), 4: (64, 192, 256, 320)}      # K / 64 below, equal to and above the stage count


def fill_class(K, nst):
    return 'below' if K // 64 < nst else 'equal' if K // 64 == nst else 'above'


# epilogue modes of gemm_nt: (epi, out16, resid, gamma); resid: None, 16 (the flavour's type) or 32
MODES = {'none32': ('none', 0, None, 0), 'none16': ('none', 1, None, 0), 'gelu32': ('gelu', 0, None, 0), 'gelu16': ('gelu', 1, None, 0),
         'res32g_32': ('resid', 0, 32, 1), 'res32g_16': ('resid', 1, 32, 1), 'res16_32': ('resid', 0, 16, 0), 'res16g_16': ('resid', 1, 16, 1)}
PAD = dict(lda=8, ldw=16, ldo=4, ldr=8, ldg=4)
DENSE = dict(lda=0, ldw=0, ldo=0, ldr=0, ldg=0)


def nt(group, M, N, K, mode, expect, tile=-1, persist=1, deep=1, pad=None, rpg=None, batch=1, slack=0):
    epi, out16, resid, gamma = MODES[mode]
    if rpg is None:
        rpg = max(1, M // 3 - 1)
    return dict(group=group, entry='nt', M=M, N=N, K=K, mode=mode, epi=epi, out16=out16, resid=resid, gamma=gamma, rpg=rpg, batch=batch, slack=slack,
                pad=dict(pad or DENSE), tile=tile, persist=persist, deep=deep, expect=tuple(expect) if isinstance(expect, tuple) else (expect, 0),
                exact=epi != 'gelu')


def qkv(group, B2, l, H, K, l2, expect, pos0=3, room=5, tile=-1, persist=1, deep=1, pad=None):
    return dict(group=group, entry='qkv', B2=B2, l=l, H=H, M=B2 * l, N=3 * H * 64, K=K, l2=l2, pos0=pos0, Lmax=pos0 + l + room, batch=1, slack=0,
                pad=dict(pad or DENSE), tile=tile, persist=persist, deep=deep, expect=tuple(expect) if isinstance(expect, tuple) else (expect, 0),
                exact=not l2, epi='qkv', out16=1, resid=None, gamma=0, rpg=1, mode=f'qkv_l2{l2}')


def name(c):
    shape = f"B2{c['B2']} l{c['l']} H{c['H']} pos{c['pos0']}/{c['Lmax']}" if c['entry'] == 'qkv' else f"b{c['batch']} rpg{c['rpg']}"
    return (f"{c['group']} {c['entry']}_{c.get('flav', '*')} {c['M']}x{c['N']}x{c['K']} {c['mode']} {shape} pad{int(any(c['pad'].values()))} "
            f"tile{c['tile']} persist{c['persist']} deep{c['deep']} -> {c['expect']}")


# ---------------------------------------------------------------------------------------------------------------------
# the table
# per instantiation: (M, N, padded) = a ragged M with N four past the tile's width, one row, one exact fit.  k_gemm16<2,2,2,2,4> runs from 256
# tiles of 64x64 on: its one row is 16388 columns wide.  The persistent kernel takes whole tiles only: 1 tile, 9 tiles (16 workgroups for 9 tiles:
# some get nothing) and 260 tiles (more than one round of 256 workgroups: the prefetch of the next tile under the epilogue)
NT_SHAPES = {K128: [(193, 132, 1), (1, 132, 0), (128, 128, 0)], K32D: [(49, 36, 1), (1, 36, 0), (32, 32, 0)],
             K64D: [(1000, 1028, 1), (1, 16388, 0), (1024, 1024, 0)], K64: [(97, 68, 1), (1, 68, 0), (64, 64, 0)],
             K192: [(289, 260, 1), (1, 260, 0), (192, 256, 0)], K256: [(385, 260, 1), (1, 260, 0), (256, 256, 0)],
             KP: [(256, 256, 1), (768, 768, 0), (16640, 1024, 0)]}
BIG_MODES = ('none16', 'res32g_32', 'gelu16')        # the 260-tile shape: three of the eight modes


def inst_cases():
    """every instantiation of gemm_nt on its three shapes under all eight epilogue / store modes, K walking through the pipeline-fill classes"""
    out = []
    for code, inst in NT_INST.items():
        ks = FILL_K[inst['nst']]
        for si, (M, N, padded) in enumerate(NT_SHAPES[code]):
            modes = BIG_MODES if M * N > 4 << 20 else tuple(MODES)
            for mi, mode in enumerate(modes):
                out.append(nt('inst', M, N, ks[(si + mi) % len(ks)], mode, code, inst['tile'], inst['persist'], inst['deep'], PAD if padded else DENSE))
    return out


def fallthrough_cases():
    """a forced 2 with persistence ON that must NOT run k_gemm16p: N % 256 != 0, rows % 256 != 0 (and both)"""
    out = []
    for M, N in ((512, 260), (385, 512), (256, 516), (257, 256)):
        for mode in ('none16', 'res32g_32', 'res16g_16'):
            out.append(nt('fallthrough', M, N, 128, mode, K256, 2, 1, 1, PAD))
    for B2, l, H in ((4, 64, 3), (3, 100, 4)):       # q/k/v: N = 576 with M = 256; N = 768 with M = 300
        out.append(qkv('fallthrough', B2, l, H, 128, 0, K256, tile=2))
    return out


# per q/k/v instantiation: (B2, l, H) = a ragged M, M = 1, an exact fit.  H 1 and 3 wherever the kernel's conditions allow; k_gemm16<2,4,2,2,3> runs
# from 256 tiles of 64x128 on (one row: 172 heads); the persistent kernel needs N = 192 H a multiple of 256 and M one of 256
QKV_SHAPES = {Q32D: [(3, 33, 3), (1, 1, 1), (2, 16, 2)], Q64D: [(33, 100, 3), (1, 1, 172), (86, 64, 2), (82, 100, 1)], Q64: [(3, 33, 3), (1, 1, 1), (2, 32, 2)],
              K128: [(3, 100, 3), (1, 1, 1), (2, 64, 2)], K192: [(3, 100, 3), (1, 1, 1), (3, 64, 4)], K256: [(3, 100, 3), (1, 1, 1), (4, 64, 4)],
              KP: [(4, 64, 4), (12, 64, 4)]}


def qkv_cases():
    out = []
    for code, inst in QKV_INST.items():
        ks = FILL_K[inst['nst']]
        for si, (B2, l, H) in enumerate(QKV_SHAPES[code]):
            for l2 in (0, 1):
                for ki in range(2):
                    out.append(qkv('qkv', B2, l, H, ks[(si + 2 * l2 + ki + (ki and 1)) % len(ks)], l2, code, pos0=3 + si, room=5 - si,
                                   tile=inst['tile'], persist=inst['persist'], deep=inst['deep'], pad=PAD if si == 0 else DENSE))
    return out


def batched_cases():
    """batch 2 and 40 (k_gemm16p: 32 / 40 workgroups per XCD clamp to 1, a workgroup then walks its XCD's whole share) with batch strides larger than
    the matrices, on every tile.  130 x 132 has 9 tiles of 64x64: 18 at batch 2 (the 32x32 kernel), 360 at batch 40 (the 64x64 one)"""
    out = []
    for code, inst in NT_INST.items():
        for batch in (2, 40):
            M, N = (130, 132)
            exp = code
            if code == KP:
                M, N = (256, 256) if batch == 2 else (768, 768)
            elif code == K64D and batch == 2:
                M, N = 520, 900
            elif code == K32D and batch == 40:
                M, N = 49, 36
            for mi, mode in enumerate(('none32', 'none16', 'gelu16')):
                if code == KP and batch == 40 and mode == 'none32':
                    continue
                out.append(nt('batched', M, N, FILL_K[inst['nst']][(mi + batch) % 3], mode, exp, inst['tile'], inst['persist'], inst['deep'],
                              PAD if code != KP else DENSE, batch=batch, slack=24))
    return out


def split_cases():
    """no forcing: split_rows16 cuts after 98304 rows (384 x 2 tiles of 256x256 = three rounds).  rows_per_group = 300 and l = 100 straddle the cut.
    N = 512: the first segment on k_gemm16p (k_gemm16<8,4,2,4> with persistence off); N = 320 (N % 256 != 0): on k_gemm16<8,4,2,4>.  The second
    segment: 128x128 from 384 tiles of 128x128 on (12288 rows at N = 512, 16384 at N = 320), the 64-row kernels below, the 32x32 kernel for a
    short one.  q/k/v: H = 4 (N = 768, cut after 65536 rows, inside image 655) and H = 3 (N = 576)"""
    out = [nt('split', 103936, 512, 64, 'res32g_32', (KP, K64D), rpg=300), nt('split', 103936, 512, 64, 'res16g_16', (K256, K64D), persist=0, rpg=300),
           nt('split', 103936, 320, 64, 'res32g_16', (K256, K64D), rpg=300, pad=PAD), nt('split', 103936, 320, 64, 'none16', (K256, K64), deep=0, rpg=300),
           nt('split', 110592, 512, 64, 'res16g_16', (KP, K128), rpg=300), nt('split', 110464, 512, 64, 'res16g_16', (KP, K64D), rpg=300),
           nt('split', 114688, 320, 64, 'res16g_16', (K256, K128), rpg=300), nt('split', 114560, 320, 64, 'res16g_16', (K256, K64D), rpg=300),
           nt('split', 101300, 320, 64, 'res32g_16', (K256, K32D), rpg=300),
           qkv('split', 700, 100, 4, 64, 0, (KP, Q64D), pos0=7, room=13), qkv('split', 700, 100, 3, 64, 0, (K256, Q64D), pos0=7, room=13),
           qkv('split', 700, 100, 4, 64, 0, (K256, Q64), pos0=7, room=13, persist=0, deep=0)]
    return out


RESID32_PAIR = []      # filled in at the end of the module


def picker_cases():
    """no forcing, K = 64: one step either side of each decision of pick_tile16 and of the small kernels' thresholds (hook and result only)"""
    return [
        # nb128 < 256 (N = 1024: 8 tiles of 128 wide): 31 x 8 = 248 -> the 64-row kernels, 32 x 8 = 256 -> the cost model (128x128)
        nt('picker', 3968, 1024, 64, 'none16', K64D), nt('picker', 4096, 1024, 64, 'none16', K128),
        # the three shapes pick_tile16's comment cites
        nt('picker', 21632, 1024, 64, 'none16', K192), nt('picker', 4608, 3072, 64, 'none16', KP), nt('picker', 8192, 1024, 64, 'none16', K128),
        # the three-way comparison, 64 rows either side of each change of its answer.  N = 1024: 128x128 -> 256x256 (one round of 256x256 against two of
        # 128x128), 256x256 -> 192x256 (t192 = 2 x 0.8625 under t128 x 0.95 = 1.767 once t256 = 2), 192x256 -> 256x256 and back (16384 rows are one
        # round of 256 tiles: the persistent kernel), 192x256 -> 256x256 (t192 3 rounds).  N = 3072 likewise, and 192x256 -> 128x128
        nt('picker', 8256, 1024, 64, 'none16', K256), nt('picker', 12096, 1024, 64, 'none16', K256), nt('picker', 12160, 1024, 64, 'none16', K192),
        nt('picker', 16384, 1024, 64, 'none16', KP), nt('picker', 16448, 1024, 64, 'none16', K192),
        nt('picker', 24576, 1024, 64, 'none16', K192), nt('picker', 24640, 1024, 64, 'none16', K256),
        nt('picker', 2688, 3072, 64, 'none16', K128), nt('picker', 2752, 3072, 64, 'none16', K256),
        nt('picker', 5376, 3072, 64, 'none16', KP), nt('picker', 5440, 3072, 64, 'none16', K192),
        nt('picker', 8064, 3072, 64, 'none16', K192), nt('picker', 8128, 3072, 64, 'none16', K128),
        # the resid32 factor (RESID32_PAIR below)
        *RESID32_PAIR,
        # batch > 1 excludes 192x256: two matrices of 10816 rows have the tile counts of 21632 rows
        nt('picker', 10816, 1024, 64, 'none16', K128, batch=2, slack=8),
        # the small kernels' own thresholds: 15 x 16 = 240 tiles of 64x64 against 256; q/k/v (H = 4: 6 tiles of 128 wide) 42 x 6 = 252 against 43 x 6 = 258
        nt('picker', 960, 1024, 64, 'res32g_16', K32D), nt('picker', 1024, 1024, 64, 'res32g_16', K64D),
        qkv('picker', 42, 64, 4, 64, 0, Q32D), qkv('picker', 43, 64, 4, 64, 0, Q64D),
    ]




def equal_groups():
    """GELU and l2norm = 1: one call (shape, mode) under every setting that can run it; all must give the same bits.  -> [(base case, [(tile, persist,
    deep, expected code)])]"""
    ragged = [(0, 1, 1, K128), (1, 1, 1, K32D), (1, 1, 0, K64), (3, 1, 1, K192), (2, 1, 1, K256), (-1, 1, 1, K32D)]
    whole = [(0, 1, 1, K128), (1, 1, 1, K64D), (1, 1, 0, K64), (3, 1, 1, K192), (2, 0, 1, K256), (2, 1, 1, KP), (-1, 1, 1, K64D)]
    qr = [(0, 1, 1, K128), (1, 1, 1, Q32D), (1, 1, 0, Q64), (3, 1, 1, K192), (2, 1, 1, K256), (-1, 1, 1, Q32D)]
    qw = [(0, 1, 1, K128), (1, 1, 1, Q64D), (1, 1, 0, Q64), (3, 1, 1, K192), (2, 0, 1, K256), (2, 1, 1, KP), (-1, 1, 1, Q64D)]
    return [(nt('equal', 300, 260, 192, 'gelu16', 0, pad=PAD), ragged), (nt('equal', 1, 260, 128, 'gelu32', 0), ragged),
            (nt('equal', 1024, 1024, 64, 'gelu16', 0), whole), (nt('equal', 1024, 1024, 192, 'gelu32', 0), whole),
            (qkv('equal', 3, 100, 3, 192, 1, 0, pad=PAD), qr), (qkv('equal', 1, 1, 3, 128, 1, 0), qr), (qkv('equal', 1, 1, 1, 64, 1, 0), qr),
            (qkv('equal', 44, 64, 4, 128, 1, 0), qw)]


GROUPS = {'inst': inst_cases, 'fallthrough': fallthrough_cases, 'qkv': qkv_cases, 'batched': batched_cases, 'split': split_cases, 'picker': picker_cases}


def cases(group=None, flav=None):
    """the table, every case in both flavours"""
    out = []
    for g, fn in GROUPS.items():
        if group is None or g == group:
            out += [dict(c, flav=f) for f in FLAVOURS if flav is None or f == flav for c in fn()]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# geometry
def geometry(c):
    """leading dimensions and batch strides in elements"""
    p, M, N, K = c['pad'], c['M'], c['N'], c['K']
    g = dict(lda=K + p['lda'], ldw=K + p['ldw'], ldo=N + p['ldo'], ldr=N + p['ldr'], ldg=N + p['ldg'])
    g['sA'], g['sW'], g['sO'] = M * g['lda'] + c['slack'], N * g['ldw'] + c['slack'], M * g['ldo'] + c['slack']
    g['G'] = (M + c['rpg'] - 1) // c['rpg']
    return g


def place(vals, ld, stride, dtype):
    """[B][R][C] values -> the flat NaN-filled buffer they occupy with leading dimension ld and batch stride `stride`"""
    B, R, C = vals.shape
    buf = torch.full(((B - 1) * stride + (R - 1) * ld + C,), NAN, dtype=dtype)
    buf.as_strided((B, R, C), (stride, ld, 1)).copy_(vals)
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# operands
def shift_of(K):
    """s of the coarse weight grid 2^-s: the K / 2 coarse products (variance 4 each) get a deviation near 8"""
    return max(0, round(math.log2(2.0 * math.sqrt(K / 2) / 8.0)))


class Operands:
    pass


_OPERANDS = {}


def operands(c):
    """grid operands of an exact case (float64 holding grid values, the same for both flavours), normal ones for GELU / l2norm = 1 (already rounded
    to the flavour).  Cached, the last few."""
    key = (c['entry'], c['M'], c['N'], c['K'], c['mode'], c['rpg'], c['batch'], c['exact'], None if c['exact'] else c['flav'])
    if key in _OPERANDS:
        return _OPERANDS[key]
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    B, M, N, K = c['batch'], c['M'], c['N'], c['K']
    o = Operands()
    if c['exact']:
        o.s = shift_of(K)
        o.A = torch.randint(-2, 3, (B, M, K), generator=g, dtype=torch.int8).float()
        wexp = torch.full((K,), float(o.s)); wexp[1::2] += FINE
        o.W = torch.randint(-2, 3, (B, N, K), generator=g, dtype=torch.int8).float() * torch.pow(2.0, -wexp)
        o.bias = torch.randint(-2048, 2049, (N,), generator=g).double() * BIAS_GRID
        o.grid = 2.0 ** -max(10, o.s + FINE)
        o.resid = o.gamma = None
        if c['resid'] == 16:
            o.resid = torch.randint(-64, 65, (M, N), generator=g, dtype=torch.int16).float() * RES16_GRID
        elif c['resid'] == 32:
            o.resid = torch.randint(-16384, 16385, (M, N), generator=g, dtype=torch.int16).float() * RES32_GRID
            o.grid = min(o.grid, RES32_GRID)
        if c['gamma']:
            G = geometry(c)['G']
            r = torch.randint(0, 16, (G, N), generator=g)
            o.gamma = ((1 - 2 * (r & 1)) * (1 + 2 * ((r >> 1) & 1))).double() * torch.pow(2.0, ((r >> 2) - 2).double())
            o.grid = o.grid / 4.0                                  # (gamma down to 2^-2)
    else:
        dt = DTYPE[c['flav']]
        o.A = (torch.randn(B, M, K, generator=g) * (0.7 if c['entry'] == 'nt' else 1.0)).to(dt).float()
        o.W = (torch.randn(B, N, K, generator=g) * ((1.5 if c['entry'] == 'nt' else 1.0) / K ** 0.5)).to(dt).float()
        o.bias = (torch.randn(N, generator=g) * (0.2 if c['entry'] == 'nt' else 0.1)).float().double()
        o.resid = o.gamma = None
        o.smul = (torch.randn(c['H'], generator=g) * 0.3 + 1.4).float() if c['entry'] == 'qkv' else None
    if len(_OPERANDS) >= 3:
        _OPERANDS.pop(next(iter(_OPERANDS)))
    _OPERANDS[key] = o
    return o


def round16(v, flav, exact=True):
    """ONE round-to-nearest-even of float64 values to the flavour's type: an exact case's value fits fp32 (asserted), so the cast through fp32 rounds once"""
    v32 = v.float()
    if exact:
        assert torch.equal(v32.double(), v), 'the exact value does not fit fp32: the cast would round twice'
    return v32.to(DTYPE[flav])


def needs_rounding(v, flav):
    """share of the float64 values v that the flavour's type cannot hold"""
    return float((round16(v, flav, exact=False).double() != v).double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# the reference.  parts(): for the rows asked for, every value a correct kernel stores and the flat element offset it stores it at; expected():
# those scattered into NaN-filled buffers.  FAULTS are what the CPU tests plant.
FAULTS = ('bias_after_round', 'resid_after_round', 'resid_through_16', 'gamma_without_bias', 'group_without_m_base', 'rpg_off_by_one',
          'qkv_pos_without_m_base', 'heads_swapped', 'kv_at_pos0_minus_1', 'ldo_as_N', 'sO_as_MN')


def applies(fault, c, cut=0):
    """does the fault concern the case?  cut: the first row of the call's second launch (0: one launch)"""
    ntc = c['entry'] == 'nt'
    return {'bias_after_round': c['exact'] and bool(c['out16']), 'resid_after_round': ntc and c['out16'] and c['resid'] is not None,
            'resid_through_16': ntc and c['resid'] == 32, 'gamma_without_bias': ntc and bool(c['gamma']),
            'group_without_m_base': ntc and bool(c['gamma']) and cut > 0, 'rpg_off_by_one': ntc and bool(c['gamma']) and c['M'] > c['rpg'],
            'qkv_pos_without_m_base': not ntc and cut > 0, 'heads_swapped': not ntc and c['H'] > 1, 'kv_at_pos0_minus_1': not ntc,
            'ldo_as_N': ntc and c['pad']['ldo'] > 0 and c['M'] > 1, 'sO_as_MN': ntc and c['batch'] > 1}[fault]


def acc64(o, rows):
    """[B][rows][N]: A W^T in float64"""
    return torch.matmul(o.A[:, rows].double(), o.W.double().transpose(1, 2))


def parts(c, flav=None, o=None, rows=None, fault=None, cut=0):
    """-> {buffer: (offsets [R][P] int64, values [R][P][W])}: value (r, p, w) is stored at flat element offsets[r][p] + w of the buffer.  Exact cases only
    (an inexact case's float64 value comes from value64)."""
    flav = flav or c['flav']
    o = o or operands(c)
    rows = torch.arange(c['M']) if rows is None else rows
    v = acc64(o, rows)
    geo = geometry(c)
    if c['entry'] == 'qkv':
        return _parts_qkv(c, flav, o, rows, v[0], fault, cut)
    rnd_any = lambda t: round16(t, flav, exact=False).double()
    cast = (lambda t: round16(t, flav)) if c['out16'] else (lambda t: _f32(t))
    late_bias = fault == 'bias_after_round'
    if not late_bias and fault != 'gamma_without_bias':
        v = v + o.bias
    if c['epi'] == 'resid':
        if o.gamma is not None:
            mg = torch.where(rows >= cut, rows - cut, rows) if fault == 'group_without_m_base' else rows
            gm = o.gamma[mg // (c['rpg'] + (fault == 'rpg_off_by_one'))]
            v = v * gm
            if fault == 'gamma_without_bias':
                v = v + o.bias
        res = o.resid[rows].double()
        if fault == 'resid_through_16':
            res = round16(res, flav, exact=False).double()
        if late_bias:
            v = round16(v + res, flav, exact=False).double() + o.bias * (gm if o.gamma is not None else 1.0)
        elif fault == 'resid_after_round':
            v = round16(v, flav, exact=False).double() + res
        else:
            v = v + res
    elif late_bias:
        v = rnd_any(v) + o.bias
    if fault in ('bias_after_round', 'resid_after_round'):
        out = round16(v, flav, exact=False) if c['out16'] else v.float()
    else:
        out = cast(v)
    ldo = c['N'] if fault == 'ldo_as_N' else geo['ldo']
    sO = c['M'] * c['N'] if fault == 'sO_as_MN' else geo['sO']
    off = (torch.arange(c['batch'])[:, None] * sO + rows[None, :] * ldo).reshape(-1, 1)
    return {'out': (off, out.reshape(-1, 1, c['N']))}


def _f32(t):
    t32 = t.float()
    assert torch.equal(t32.double(), t), 'the exact value does not fit fp32'
    return t32


def _parts_qkv(c, flav, o, rows, v, fault, cut):
    H, l, C, Lmax = c['H'], c['l'], c['H'] * 64, c['Lmax']
    if fault == 'bias_after_round':
        v = round16(v, flav, exact=False).double() + o.bias
    else:
        v = v + o.bias
    v = v.view(-1, 3, H, 64)
    q = v[:, 0] * Q_PLAIN
    vals = [round16(t, flav, exact=fault is None) for t in (q, v[:, 1], v[:, 2])]
    heads = torch.arange(H)
    hd = (H - 1 - heads) if fault == 'heads_swapped' else heads
    mp = torch.where(rows >= cut, rows - cut, rows) if fault == 'qkv_pos_without_m_base' else rows
    bb, t = mp // l, mp % l
    pos0 = c['pos0'] - (fault == 'kv_at_pos0_minus_1')
    qoff = rows[:, None] * C + hd[None, :] * 64
    coff = ((bb[:, None] * H + hd[None, :]) * Lmax + pos0 + t[:, None]) * 64
    return {'q': (qoff, vals[0]), 'kc': (coff, vals[1]), 'vc': (coff, vals[2])}


def buffer_sizes(c):
    geo = geometry(c)
    if c['entry'] == 'qkv':
        return {'q': c['M'] * c['H'] * 64, 'kc': c['B2'] * c['H'] * c['Lmax'] * 64, 'vc': c['B2'] * c['H'] * c['Lmax'] * 64}
    return {'out': (c['batch'] - 1) * geo['sO'] + (c['M'] - 1) * geo['ldo'] + c['N']}


def out_dtype(c, flav):
    return DTYPE[flav] if c['out16'] else torch.float32


def scatter(c, flav, pts):
    """the parts in NaN-filled buffers of the sizes the call is given"""
    out = {}
    for nm, n in buffer_sizes(c).items():
        off, vals = pts[nm]
        buf = torch.full((n,), NAN, dtype=vals.dtype)
        W = vals.shape[-1]
        flat = off.reshape(-1)
        step = int(flat[1] - flat[0]) if flat.numel() > 1 else W
        if flat.numel() > 1 and step >= W and bool((flat[1:] - flat[:-1] == step).all()):
            buf.as_strided((flat.numel(), W), (step, 1), int(flat[0])).copy_(vals.reshape(-1, W))
        else:
            buf[(flat[:, None] + torch.arange(W)[None, :]).reshape(-1)] = vals.reshape(-1)
        out[nm] = buf
    return out


def expected(c, o=None):
    """{buffer: the flat buffer a correct kernel leaves behind, NaN where it stores nothing}"""
    return scatter(c, c['flav'], parts(c, c['flav'], o))


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def exactness_budget(c, o=None, rows=None):
    """the largest |partial sum| any summation order can meet, in units of the finest grid: (|A| |W|^T + |bias|) |gamma| + |resid|"""
    o = o or operands(c)
    rows = torch.arange(c['M']) if rows is None else rows
    v = torch.matmul(o.A[:, rows].double().abs(), o.W.double().abs().transpose(1, 2)) + o.bias.abs()
    if o.gamma is not None:
        v = v * o.gamma[rows // c['rpg']].abs()
    if o.resid is not None:
        v = v + o.resid[rows].double().abs()
    return float(v.max()) / o.grid


def before_resid(c, o=None, rows=None):
    """gamma (acc + bias): the value an fp32 RESID store adds the residual to"""
    o = o or operands(c)
    rows = torch.arange(c['M']) if rows is None else rows
    v = acc64(o, rows) + o.bias
    return v * o.gamma[rows // c['rpg']] if o.gamma is not None else v


def probe_rows(c, cut=0):
    """the rows the CPU tests evaluate of a large case: the first and last 300 and 300 / 600 either side of the cut"""
    M = c['M']
    if M <= 4096:
        return torch.arange(M)
    r = [torch.arange(300), torch.arange(M - 300, M)]
    if cut:
        r.append(torch.arange(cut - 300, cut + 600))
    return torch.unique(torch.cat(r))


# ---------------------------------------------------------------------------------------------------------------------
# GELU and l2norm = 1: float64 values and the existing bars
def value64(c, o=None):
    """nt + GELU: [B][M][N]; q/k/v with l2norm = 1: (q [M][H][64], k, v)"""
    o = o or operands(c)
    v = acc64(o, torch.arange(c['M'])) + o.bias
    if c['entry'] == 'nt':
        return torch.nn.functional.gelu(v, approximate='tanh')
    v = v[0].view(-1, 3, c['H'], 64)
    q, k = v[:, 0], v[:, 1]
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12) * o.smul.double().clamp_max(math.log(100)).exp().view(1, -1, 1)
    k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return q, k, v[:, 2]


def mag64(c, o=None):
    o = o or operands(c)
    return torch.matmul(o.A.double().abs(), o.W.double().abs().transpose(1, 2))


def qkv_tolerance(ref, flav):
    """tests/test_f16_gpu.py::test_gemm_qkv16_against_float64 / tests/test_bf16_gpu.py: one 16-bit rounding + 2e-4"""
    return ref.abs() * ULP16[flav] + 2e-4


# ---------------------------------------------------------------------------------------------------------------------
# the resid32 factor of pick_tile16 decides only where t256 and the best of t128 / t192 are within 5 %: five rounds of 256x256 (x 0.95 = 4.75)
# against eight rounds of 128x128 (x 0.62 = 4.96).  154000 x 260: 602 x 2 = 1204 tiles of 256x256 (five rounds, the last 70.3 % full: no split),
# 1204 x 3 = 3612 of 128x128 (eight rounds of 512), 803 x 2 of 192x256 (seven rounds = 6.04): 256x256 with an fp32 residual, 128x128 without.
RESID32_PAIR += [nt('picker', 154000, 260, 64, 'res32g_32', K256, rpg=300), nt('picker', 154000, 260, 64, 'res16g_16', K128, rpg=300)]
