"""One case table, one operand builder and one float64 reference for the 16-bit 3x3 convolutions of var_amd/csrc/conv16.hip
(varhip_conv3x3_nhwc_*, varhip_gnconv3x3_nhwc_*, varhip_upconv_phase_*), shared by tests/test_conv16_dispatch_cpu.py (the table, the
conditions on its operands and the planted faults, no GPU) and tests/test_conv16_dispatch_gpu.py (every instantiation on the GPU).

Cases.  A case names the entry point ('conv', 'gnconv', 'upconv'), the flavour, B, H, W (the map the call is given: the OUTPUT map for
'upconv'), Cin, Cout, the residual, out_mode, the forced tile `wm` (0: the automatic picker) and `expect`, the value
varhip_conv16_last_pick() must return after the call (include/var_hip.h: nz * 1000 + GN * 100 + TNW * 10 + kernel).  `expect` is written
down per group of the table from the kernel the group is built for; tests/test_conv16_dispatch_cpu.py restates pick_conv16 and the choice
of dispatch_conv16 on its own and compares.

Operands of the 'conv' and 'upconv' cases lie on a dyadic grid: activations are integers in [-2, 2], weights integers in [-2, 2] times
2^-s, the bias fp32 multiples of 2^-10, the residual multiples of 2^-4 in [-4, 4] (all exact in fp16 and in bfloat16, so both flavours get
the same operands).  Every product and every partial sum of products, bias and residual, in ANY order, is a multiple of the finest grid in
use and stays below 2^24 units of it (exactness_budget, asserted): exact in fp32.  Whatever its K order, a correct kernel therefore holds
the exact value in fp32 and rounds it ONCE to the output type, and the expectation is conv2d in float64, plus bias and residual, cast
once (the exact value fits fp32, so the cast through fp32 rounds once) — compared with torch.equal.  out_mode 1 / 2 keep fp32: the clamp
is exact and (x + 1) * 0.5 of a multiple of 2^-10 in [0, 2] is exact.

s is chosen per case from K = taps * Cin and the out_mode alone.  For the 16-bit stores the weights of the even input channels use 2^-s
and those of the odd ones 2^-(s + 8): a sum of K / 2 products has the standard deviation 2 sqrt(K / 2) (activations and weight numerators
both have variance 2), a few dozen units, so with ONE grid the convolution alone would always fit the 11 bits of fp16 and a kernel that
rounded it before adding the bias or the residual would go unseen.  With the two grids eight bits apart the convolution alone needs up to
15 bits, s puts the coarse half's deviation near 8, and the bias reaches down to 2^-10: the sum before the bias, the sum before the
residual and the final value each need a real rounding.  For out_mode 1 / 2 (no rounding anywhere) one grid, its deviation between
0.4 and 0.8, and |bias| <= 0.5: most results stay inside the clamp, some reach it on either side.

The 'gnconv' cases cannot be dyadic (the normalisation is not); they keep the criterion of
tests/test_f16_gpu.py::test_gnconv16_fused_equals_apply_then_conv, whose tolerance gn_tolerance restates."""
import math
import zlib

import torch

FLAVOURS = ('f16', 'bf16')
DTYPE = {'f16': torch.float16, 'bf16': torch.bfloat16}
BIAS_GRID = 2.0 ** -10
FINE = 8                                             # the odd input channels' weights lie on a grid 2^-FINE finer than the even ones' (16-bit stores)
SENTINEL32 = 7.0                                     # fill of the fp32 NCHW outputs: the clamp to [-1, 1] (and its image [0, 1]) cannot produce it
K128, K256, KH32, KH16 = 0, 3, 1, 2                  # the kernel digit of varhip_conv16_last_pick


def hook(kernel, tnw, gn=0, nz=1):
    return nz * 1000 + gn * 100 + tnw * 10 + kernel


def case(group, entry, B, H, W, Cin, Cout, res=0, omode=0, wm=0, expect=None, silu=1, einval=False):
    return dict(group=group, entry=entry, B=B, H=H, W=W, Cin=Cin, Cout=Cout, res=res, omode=omode, wm=wm, expect=expect, silu=silu, einval=einval)


def name(c):
    return (f"{c['group']} {c['entry']}_{c.get('flav', '*')} B{c['B']} {c['H']}x{c['W']} {c['Cin']}->{c['Cout']} res{c['res']} omode{c['omode']} "
            f"wm{c['wm']} -> {c['expect']}")


# ---------------------------------------------------------------------------------------------------------------------
# the table
# k_conv16h: (B, H, W, Cin, channel tiles); workgroups = patches * channel tiles, dealt to 8 XCDs: q = wgs >> 3, rem = wgs & 7
HALO_SHAPES = {
    32: [(2, 8, 32, 32, 1),          # one channel tile, one 8 x 32 patch per image: 2 workgroups
         (1, 16, 64, 64, 2),         # two channel tiles, 4 patches: 8 workgroups, rem = 0
         (3, 8, 32, 96, 3),          # three channel tiles, one patch per image: 9 workgroups, q = 1, rem = 1
         (2, 16, 32, 160, 1)],       # 5 chunks (the decoder's own count), 4 patches; 16 x 32 also tiles into 16 x 16 patches: 8 x 32 must win
    16: [(2, 16, 16, 32, 1),
         (1, 64, 16, 64, 2),         # 4 patches x 2 channel tiles: 8 workgroups, rem = 0
         (3, 16, 16, 96, 3),         # 9 workgroups
         (1, 16, 48, 160, 1),        # W % 32 != 0: the 16 x 16 form by geometry, 3 patches
         (1, 16, 48, 32, 2)],        # the same map with two channel tiles: 6 workgroups, q = 0, rem = 6
}
TILE_COUTS = {5: (160, 320, 640), 4: (128, 256, 384), 2: (64, 192), 1: (32, 96, 36, 100, 200, 6, 30, 3)}      # k_conv16<TNW, ..>: Cout (640 = 4 * 160 = 5 * 128 takes TNW 5)
# k_conv16 pixel counts: one 128-pixel tile; two 256-pixel tiles (2 chunks); one image and three images inside one tile; 270 pixels (an image and a
# tile boundary that do not coincide); five 64-pixel images on 320 pixels (a partial third 128-pixel tile, a partial second 256-pixel one)
TILE_SHAPES = [(1, 8, 16, 32), (2, 16, 16, 64), (1, 5, 7, 32), (3, 5, 7, 32), (2, 9, 15, 32), (5, 8, 8, 32)]
PHASE_COUTS = {5: (160,), 4: (256,), 2: (192,), 1: (96, 36)}
PHASE_SHAPES = [(1, 6, 10, 32), (3, 6, 10, 32), (2, 16, 16, 32), (2, 32, 32, 64)]      # OUTPUT maps: 3 x 5 low-resolution maps (odd), 128 and 512 low-resolution pixels


def halo_cases():
    """k_conv16h<TNW, PW, false> through conv3x3_nhwc with wm = 8: every shape of HALO_SHAPES at TNW 5 and 4, with and without a residual,
    and Cout = 640 (a multiple of 160 AND of 128: TNW 5)"""
    out = []
    for pw, kern in ((32, KH32), (16, KH16)):
        for tnw in (5, 4):
            for B, H, W, Cin, tiles in HALO_SHAPES[pw]:
                for res in (0, 1):
                    out.append(case('halo', 'conv', B, H, W, Cin, tnw * 32 * tiles, res, 0, 8, hook(kern, tnw)))
        B, H, W, Cin, _ = HALO_SHAPES[pw][0]
        out.append(case('halo', 'conv', 1, H, W, Cin, 640, 1, 0, 8, hook(kern, 5)))
    return out


def gn_cases():
    """k_conv16h<TNW, PW, true> through gnconv3x3_nhwc (and <.., false> through the two launches it must equal), the same shapes; the residual
    and SiLU alternate; one shape varhip_conv16_gn_fusable refuses: the table of 640 channels does not fit beside 8 x 32 patches"""
    out = []
    for pw, kern in ((32, KH32), (16, KH16)):
        for tnw in (5, 4):
            for i, (B, H, W, Cin, tiles) in enumerate(HALO_SHAPES[pw]):
                out.append(case('gn', 'gnconv', B, H, W, Cin, tnw * 32 * tiles, (i + tnw) & 1, 0, 8, hook(kern, tnw, gn=1), silu=int(i != 2)))
    out.append(case('gn', 'gnconv', 1, 8, 32, 640, 160, 1, 0, 8, None, einval=True))
    return out


def tile_cases():
    """k_conv16<TNW, ..> on 128-pixel (wm = 2) and 256-pixel (wm = 4) tiles, 16-bit NHWC store: every Cout of TILE_COUTS on every pixel count of
    TILE_SHAPES, with and without a residual.  TNW 2 and 1 have no 256-pixel form: wm = 4 must still run (and report) the 128-pixel kernel"""
    out = []
    for tnw, couts in TILE_COUTS.items():
        for Cout in couts:
            for B, H, W, Cin in (TILE_SHAPES if Cout != 640 else TILE_SHAPES[:1] + TILE_SHAPES[4:5]):
                for wm in (2, 4):
                    for res in (0, 1):
                        out.append(case('tile', 'conv', B, H, W, Cin, Cout, res, 0, wm, hook(K256 if wm == 4 and tnw >= 4 else K128, tnw)))
    return out


def omode_cases():
    """the fp32 NCHW stores of the element-wise epilogue (out_mode 1: de-normalised, 2: clamped) at Cout 3, 4 and 8 (4 and 8 would take the vector
    epilogue with out_mode 0)"""
    out = []
    for Cout in (3, 4, 8):
        for B, H, W, Cin in ((1, 8, 16, 32), (3, 5, 7, 64), (2, 9, 15, 32)):
            for omode in (1, 2):
                for wm in (2, 4):
                    out.append(case('omode', 'conv', B, H, W, Cin, Cout, 0, omode, wm, hook(K128, 1)))
    return out


def phase_cases():
    """every k_conv16 instantiation in its nz = 4 phase form (upconv_phase: the map named is the OUTPUT)"""
    out = []
    for tnw, couts in PHASE_COUTS.items():
        for Cout in couts:
            for B, H, W, Cin in PHASE_SHAPES:
                for wm in (2, 4):
                    out.append(case('phase', 'upconv', B, H, W, Cin, Cout, 0, 0, wm, hook(K256 if wm == 4 and tnw >= 4 else K128, tnw, nz=4)))
    return out


def auto_cases():
    """no forcing: one step of B on either side of each threshold of pick_conv16.  The halo-patch kernel from (M / 256) * (N / BN) >= 256 on
    (8 x 32 maps, Cout 160: B = 256 against 255, which has 255 256-pixel tiles and so takes the 128-pixel ones); the 256-pixel tiles from
    ceil(M / 256) * ceil(N / 160) * nz >= 256 on, on 12 x 20 maps that tile into no patch (B = 273: 65520 pixels = 256 tiles; B = 272: 255) and
    in the phase form (32 x 32 output = 256 low-resolution pixels per image, nz = 4: B = 64 against 63).  They say nothing about speed."""
    return [case('auto', 'conv', 256, 8, 32, 32, 160, 1, 0, 0, hook(KH32, 5)), case('auto', 'conv', 255, 8, 32, 32, 160, 1, 0, 0, hook(K128, 5)),
            case('auto', 'conv', 273, 12, 20, 32, 160, 0, 0, 0, hook(K256, 5)), case('auto', 'conv', 272, 12, 20, 32, 160, 0, 0, 0, hook(K128, 5)),
            case('auto', 'upconv', 64, 32, 32, 32, 160, 0, 0, 0, hook(K256, 5, nz=4)), case('auto', 'upconv', 63, 32, 32, 32, 160, 0, 0, 0, hook(K128, 5, nz=4))]


GROUPS = {'halo': halo_cases, 'gn': gn_cases, 'tile': tile_cases, 'omode': omode_cases, 'phase': phase_cases, 'auto': auto_cases}


def cases(group=None, flav=None):
    """the table, every case in both flavours"""
    out = []
    for g, fn in GROUPS.items():
        if group is None or g == group:
            out += [dict(c, flav=f) for f in FLAVOURS if flav is None or f == flav for c in fn()]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# dyadic operands and the exact reference
def shift_of(c):
    """s of the weight grid 2^-s, from K = taps * Cin and the out_mode alone (module docstring)"""
    K = (4 if c['entry'] == 'upconv' else 9) * c['Cin']
    if c['omode'] == 0:
        K //= 2                                                    # (the coarse half of the input channels carries the magnitude)
    target = 8.0 if c['omode'] == 0 else 0.8
    s = math.log2(2.0 * math.sqrt(K) / target)
    return max(0, min(10, round(s) if c['omode'] == 0 else math.ceil(s)))


_OPERANDS = {}


class Operands:
    pass


def operands(c):
    """x [B][h][w][Cin], w [Cout][3][3][Cin] ('upconv': the packed phase weights [4][Cout][2][2][Cin], h, w the low-resolution map), bias [Cout],
    resid [B][H][W][Cout] or None, all float64 holding grid values; the same for both flavours and every forced tile (cached, the last few)"""
    key = (c['entry'], c['B'], c['H'], c['W'], c['Cin'], c['Cout'], c['res'], c['omode'])
    if key in _OPERANDS:
        return _OPERANDS[key]
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    up = c['entry'] == 'upconv'
    h, w = (c['H'] // 2, c['W'] // 2) if up else (c['H'], c['W'])
    o = Operands()
    o.s = shift_of(c)
    o.x = torch.randint(-2, 3, (c['B'], h, w, c['Cin']), generator=g).double()
    wshape = (4, c['Cout'], 2, 2, c['Cin']) if up else (c['Cout'], 3, 3, c['Cin'])
    o.wnum = torch.randint(-2, 3, wshape, generator=g).double()
    o.wexp = torch.full((c['Cin'],), float(o.s), dtype=torch.float64)
    if c['omode'] == 0:
        o.wexp[1::2] += FINE                                       # (the fine half of the input channels: module docstring)
    o.w = o.wnum * torch.pow(2.0, -o.wexp)
    o.grid = 2.0 ** -max(10.0, float(o.wexp.max()))
    span = 2048 if c['omode'] == 0 else 512                      # |bias| <= 2 (out_mode 0), <= 0.5 (the clamped stores)
    o.bias = torch.randint(-span, span + 1, (c['Cout'],), generator=g).double() * BIAS_GRID
    o.resid = torch.randint(-64, 65, (c['B'], c['H'], c['W'], c['Cout']), generator=g).double() / 16.0 if c['res'] else None
    if len(_OPERANDS) >= 4:
        _OPERANDS.pop(next(iter(_OPERANDS)))
    _OPERANDS[key] = o
    return o


def conv64(c, x, w, padded=None):
    """the convolution alone in float64 -> [B][H][W][Cout] (channels last, as the kernels store it).  padded: the 3x3 form's input with its one-pixel
    border already in place, [B][Cin][H + 2][W + 2] (the planted faults of the CPU tests build their own)"""
    F = torch.nn.functional
    if c['entry'] == 'upconv':
        xd = x.permute(0, 3, 1, 2)
        ref = torch.empty(c['B'], c['Cout'], c['H'], c['W'], dtype=torch.float64)
        for py in range(2):
            for px in range(2):
                k = w[py * 2 + px].permute(0, 3, 1, 2)                              # [Cout][Cin][2][2]
                xp = F.pad(xd, (1 - px, px, 1 - py, py))                           # taps (a, b) read low-res pixel (y + a - 1 + py, x + b - 1 + px)
                ref[:, :, py::2, px::2] = F.conv2d(xp, k)
        return ref.permute(0, 2, 3, 1).contiguous()
    if padded is None:
        padded = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
    return F.conv2d(padded, w.permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous()


def round16(v, flav, exact=True):
    """ONE round-to-nearest-even of float64 grid values to the flavour's type: the value is exact in fp32 (asserted), so the cast through fp32 rounds once"""
    v32 = v.float()
    if exact:
        assert torch.equal(v32.double(), v), 'the exact value does not fit fp32: the cast would round twice'
    return v32.to(DTYPE[flav])


def finish(c, flav, acc, bias, resid):
    """what a correct kernel stores for the exact convolution acc [B][H][W][Cout]: out_mode 0 -> the 16-bit NHWC map; 1 / 2 -> fp32 NCHW"""
    v = acc + bias
    if resid is not None:
        v = v + resid
    if c['omode'] == 0:
        return round16(v, flav)
    v = v.clamp(-1.0, 1.0)
    if c['omode'] == 1:
        v = (v + 1.0) * 0.5
    v32 = v.float()
    assert torch.equal(v32.double(), v)
    return v32.permute(0, 3, 1, 2).contiguous()


def expected(c, o=None):
    o = o or operands(c)
    return finish(c, c['flav'], conv64(c, o.x, o.w), o.bias, o.resid)


def exactness_budget(c, o=None):
    """the largest |partial sum| any summation order can meet, in units of the grid: conv(|x|, |w|) + |bias| + |resid|"""
    o = o or operands(c)
    v = conv64(c, o.x.abs(), o.w.abs()) + o.bias.abs()
    if o.resid is not None:
        v = v + o.resid.abs()
    return float(v.max()) / o.grid


def needs_rounding(v, flav):
    """share of the float64 values v that the flavour's type cannot hold"""
    return float((round16(v, flav, exact=False).double() != v).double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# what remains of the tolerance formulas (the GroupNorm-fused cases and the GroupNorm partials), restated once
def gn_tolerance(ref, Cin, flav):
    """tests/test_f16_gpu.py::test_gnconv16_fused_equals_apply_then_conv, unchanged: one 16-bit rounding of the result (2^-10 relative in fp16, 2^-7
    in bfloat16, tests/test_bf16_gpu.py's ULP) and fp32 accumulation noise over 9 Cin terms"""
    return 1e-5 + ref.abs() * 2.0 ** (-10 if flav == 'f16' else -7) + 4e-6 * (9 * Cin) ** 0.5


PART_BLOCK = dict(rtol=1e-5, atol=1e-4)              # k_conv16's GroupNorm partials against the sums of the rounded outputs, per block of 128 pixels (test_conv16_against_float64)
PART_SAMPLE = dict(rtol=1e-5, atol=1e-3)             # k_conv16h's (and the phase form's), per sample: its blocks are halves of 2-D patches
