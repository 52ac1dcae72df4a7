"""The VAE's row and element-wise kernels on an MI355X against the float64 references and derived bars of tests/rowcases.py, on every geometry and
value regime of its decks, every operand inside a guard arena (tests/util.py).  Each test prints `max err / bar` per case (pytest -s);
profiles/rowops_bar_margins.txt is a record of those lines.

fp32 contracts with the oracle's twin are kept on the new geometries: gn_apply_f32 without SiLU, softmax_rows_f32 and the layout copies are
bit-equal to it; the fp32 statistics (float64 sums in another order) stay within atol 1e-6 / rtol 2e-6 of it and get the float64 bar on top.

varhip_gn_scale_shift_f32 and k_gn16_apply form shift = beta - mean * scale.  The library is built with -ffp-contract=off, and the gfx950 code of
both kernels (llvm-objdump -d of the code object: k_gn_scale_shift is v_mul_f32, v_mul_f32, v_sub_f32; k_gn16_apply has v_pk_mul_f32 for the
two products, v_pk_add_f32 with a negated operand for the difference, and v_pk_fma_f32 only for the eight x * sc + sh it writes as fma) rounds
the product and the difference SEPARATELY: no fused multiply-add.  rowcases.emu_scale_shift evaluates exactly that in numpy float32 and the
table must equal it bit for bit; the CPU test shows the deck tells the two forms apart."""
import numpy as np
import pytest

from tests import rowcases as rc
from tests import util

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
FLAVS = ('f32', 'f16', 'bf16')
SENTINEL = 0x5A5A5A5A


def _setup():
    util.ensure_oracle_built()
    from oracle import var_oracle
    from var_amd import hip
    return var_oracle.lib(), hip


def dev(a, flav='f32'):
    """numpy values (exact in the flavour) -> device tensor of the flavour"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(rc.torch_dtype(flav)).cuda()


def nans(shape, flav='f32'):
    return torch.full(shape, float('nan'), dtype=rc.torch_dtype(flav), device='cuda')


def host64(t):
    return t.double().cpu().numpy()


def twin(name, *args):
    L, _ = _setup()
    assert util.guarded_invoke(f'varref_{name}', list(args), L[name]) == 0


def report(tag, got, ref, bar):
    m = rc.margin(got, ref, bar)
    print(f'{tag}: max err / bar = {m:.4f}')
    assert m <= 1.0, f'{tag}: max err / bar = {m:.4g}'


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def refused(name, args):
    """the entry point called directly (hip.call raises): VARHIP_EINVAL, nothing written"""
    _, hip = _setup()
    from var_amd import abi
    rcode = util.guarded_invoke(f'varhip_{name}', args, lambda *a: hip.lib().fn[name](*a, hip.current_stream()), torch.cuda.synchronize)
    assert rcode == abi.EINVAL, f'{name}: rc={rcode}'


# ---------------------------------------------------------------------------------------------------------------------
def _gn_ids():
    return [pytest.param(flav, geo, regime, id=f'{flav} {cid}') for flav in FLAVS for cid, geo, regime in rc.gn_cases(flav)]


@pytest.mark.parametrize('flav,geo,regime', _gn_ids())
def test_groupnorm(flav, geo, regime):
    """statistics against the float64 moments of the map, then apply (without and with SiLU) on the kernel's own statistics against
    (x - mean) rstd gamma + beta in float64"""
    _, hip = _setup()
    B, HW, C, G = geo
    b = rc.build_gn(flav, geo, regime)
    tag = f'gn {flav} {regime} {B}-{HW}-{C}-{G}'
    x = dev(b.x, flav)
    stats = nans((B, G, 2))
    scratch = torch.empty(hip.gn_scratch_elems(B, HW, C, G), dtype=torch.float64, device='cuda')
    util.guarded_call('gn_stats_' + flav, x, stats, scratch, B, HW, C, G, rc.EPS)
    st = stats.cpu().numpy()
    mean, var = rc.gn_moments64(b.x, G)
    bm, br = rc.bar_stats(mean, var, HW * (C // G))
    report(tag + ' mean', st[..., 0], mean, bm)
    report(tag + ' rstd', st[..., 1], 1 / np.sqrt(var + rc.EPS), br)
    x32 = b.x.astype(np.float32)
    if flav == 'f32':
        want = np.zeros((B, G, 2), np.float32)
        twin('gn_stats_f32', x32, want, np.zeros(B * G * 2, np.float64), B, HW, C, G, rc.EPS)
        ok, msg = util.diff_report(tag + ' stats vs twin', st, want, atol=1e-6, rtol=2e-6)
        assert ok, msg
    m32, r32 = st[..., 0].astype(np.float64), st[..., 1].astype(np.float64)
    gamma, beta = dev(b.gamma), dev(b.beta)
    for silu in (0, 1):
        out = nans((B, HW, C), flav)
        util.guarded_call('gn_apply_' + flav, x, stats, gamma, beta, out, B, HW, C, G, silu)
        report(f'{tag} apply silu={silu}', host64(out), rc.gn_apply64(b.x, m32, r32, b.gamma, b.beta, silu),
               rc.bar_apply(flav, b.x, m32, r32, b.gamma, b.beta, silu))
        if flav == 'f32' and not silu:
            want = np.zeros((B, HW, C), np.float32)
            twin('gn_apply_f32', x32, st, b.gamma, b.beta, want, B, HW, C, G, 0)
            assert np.array_equal(bits32(out.cpu().numpy()), bits32(want)), tag + ': gn_apply_f32 differs from the twin'


@pytest.mark.parametrize('case', [c for _, c in rc.PART_CASES], ids=[i for i, _ in rc.PART_CASES])
def test_gn_stats_from_partials(case):
    B, nblk, HW, C, G = case
    x, part = rc.build_part(case)
    stats = nans((B, G, 2))
    util.guarded_call('gn_stats_part_f32', torch.from_numpy(part).cuda(), stats, B, nblk, HW, C, G, rc.EPS)
    st = stats.cpu().numpy()
    mean, var = rc.gn_moments64(x, G)
    bm, br = rc.bar_stats(mean, var, HW * (C // G))
    tag = 'gn %s' % (rc.PART_CASES[[c for _, c in rc.PART_CASES].index(case)][0])
    report(tag + ' mean', st[..., 0], mean, bm)
    report(tag + ' rstd', st[..., 1], 1 / np.sqrt(var + rc.EPS), br)
    want = np.zeros((B, G, 2), np.float32)
    twin('gn_stats_part_f32', part, want, B, nblk, HW, C, G, rc.EPS)
    ok, msg = util.diff_report(tag + ' vs twin', st, want, atol=1e-6, rtol=2e-6)
    assert ok, msg


@pytest.mark.parametrize('case', rc.SCALE_SHIFT_CASES, ids=lambda c: 'B=%d C=%d G=%d' % c)
def test_gn_scale_shift(case):
    """the table against float64, bit-equal to the separately rounded float32 evaluation (module docstring), and bit-equal to what k_gn16_apply
    forms for itself: gn_apply_<f16|bf16> without SiLU returns round16(sh) at x = 0 and round16(fl32(sc + sh)) at x = 1"""
    B, C, G = case
    stats, gamma, beta = rc.build_scale_shift(case)
    table = nans((B, 2, C))
    dstats, dgamma, dbeta = dev(stats), dev(gamma), dev(beta)
    util.guarded_call('gn_scale_shift_f32', dstats, dgamma, dbeta, table, B, C, G)
    t = table.cpu().numpy()
    m, r = stats[..., 0].astype(np.float64), stats[..., 1].astype(np.float64)
    bsc, bsh = rc.bar_scale_shift(m, r, gamma, beta, C)
    tag = 'gn_scale_shift B=%d C=%d G=%d' % case
    report(tag + ' scale', t[:, 0], rc.per_channel(r, C)[:, 0] * gamma.astype(np.float64), bsc[:, 0])
    report(tag + ' shift', t[:, 1], beta.astype(np.float64) - rc.per_channel(m, C)[:, 0] * t[:, 0].astype(np.float64), bsh[:, 0])
    assert np.array_equal(bits32(t), bits32(rc.emu_scale_shift(stats, gamma, beta))), tag + ': not the separately rounded float32 evaluation'
    if C % 8 == 0:
        for flav in ('f16', 'bf16'):
            x = torch.zeros((B, 2, C), dtype=rc.torch_dtype(flav), device='cuda')
            x[:, 1] = 1.0
            out = nans((B, 2, C), flav)
            util.guarded_call('gn_apply_' + flav, x, dstats, dgamma, dbeta, out, B, 2, C, G, 0)
            got = out.view(torch.int16).cpu().numpy().view(np.uint16)
            assert np.array_equal(got[:, 0], rc.cast_to16(flav, t[:, 1])), f'{tag}: gn_apply_{flav} forms another shift'
            assert np.array_equal(got[:, 1], rc.cast_to16(flav, (t[:, 0] + t[:, 1]).astype(np.float32))), f'{tag}: gn_apply_{flav} forms another scale'


@pytest.mark.parametrize('flav', FLAVS)
@pytest.mark.parametrize('geo', [(1, 257, 96, 32), (2, 64, 640, 32)], ids=lambda g: '%d-%d-%d-%d' % g)
def test_groupnorm_composite(flav, geo):
    """stats -> gn_scale_shift -> apply against torch's group_norm (+ SiLU) in float64 end to end, the statistics' own bars propagated into the bar"""
    _, hip = _setup()
    B, HW, C, G = geo
    b = rc.build_gn(flav, geo, 'randn')
    x = dev(b.x, flav)
    stats, table = nans((B, G, 2)), nans((B, 2, C))
    scratch = torch.empty(hip.gn_scratch_elems(B, HW, C, G), dtype=torch.float64, device='cuda')
    gamma, beta = dev(b.gamma), dev(b.beta)
    util.guarded_call('gn_stats_' + flav, x, stats, scratch, B, HW, C, G, rc.EPS)
    util.guarded_call('gn_scale_shift_f32', stats, gamma, beta, table, B, C, G)
    assert np.array_equal(bits32(table.cpu().numpy()), bits32(rc.emu_scale_shift(stats.cpu().numpy(), b.gamma, b.beta)))
    mean, var = rc.gn_moments64(b.x, G)
    rstd = 1 / np.sqrt(var + rc.EPS)
    extra = rc.bar_propagated(b.x, mean, rstd, b.gamma, *rc.bar_stats(mean, var, HW * (C // G)))
    ref = torch.nn.functional.group_norm(torch.from_numpy(b.x).permute(0, 2, 1), G, torch.from_numpy(b.gamma).double(), torch.from_numpy(b.beta).double(),
                                         eps=rc.EPS).permute(0, 2, 1)
    for silu in (0, 1):
        out = nans((B, HW, C), flav)
        util.guarded_call('gn_apply_' + flav, x, stats, gamma, beta, out, B, HW, C, G, silu)
        want = (torch.nn.functional.silu(ref) if silu else ref).numpy()
        report(f'gn composite {flav} {B}-{HW}-{C}-{G} silu={silu}', host64(out), want, rc.bar_apply(flav, b.x, mean, rstd, b.gamma, b.beta, silu, extra=extra))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', rc.SOFTMAX_CASES, ids=rc.softmax_id)
def test_softmax_rows(case):
    rows, n, kind, scale = case
    x = rc.build_softmax(case)
    out = nans((rows, n))
    util.guarded_call('softmax_rows_f32', torch.from_numpy(x).cuda(), out, rows, n, scale)
    got = out.cpu().numpy()
    want = np.zeros_like(x)
    twin('softmax_rows_f32', x, want, rows, n, scale)
    assert np.array_equal(bits32(got), bits32(want)), 'softmax_rows_f32 differs from the twin'
    report('softmax ' + rc.softmax_id(case), got, rc.softmax_rows64(x, scale), rc.bar_softmax(x, scale))


@pytest.mark.parametrize('n', rc.SOFTMAX_REFUSED)
def test_softmax_rows_refuses(n):
    x = torch.zeros(4 * 1025, device='cuda')
    out = torch.full((4 * 1025,), SENTINEL, dtype=torch.int32, device='cuda')
    refused('softmax_rows_f32', [x, out.view(torch.float32), 4, n, 1.0])
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', rc.LAYOUT_CASES, ids=lambda c: 'B=%d C=%d HW=%d' % c)
def test_layout_copies(case):
    """bit for bit against numpy's transpose and against the twin, on arbitrary bit patterns; the pad lanes are written as +0"""
    B, C, HW = case
    bits = rc.build_layout(case)
    src = torch.from_numpy(bits.view(np.int32)).cuda().view(torch.float32)
    fresh = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)
    got = lambda t: t.view(torch.int32).cpu().numpy().view(np.uint32)
    nhwc = fresh(B, HW, C)
    util.guarded_call('nchw_to_nhwc_f32', src, nhwc, B, C, HW)
    assert np.array_equal(got(nhwc), rc.nchw_to_nhwc(bits))
    w = np.zeros((B, HW, C), np.float32)
    twin('nchw_to_nhwc_f32', bits.view(np.float32), w, B, C, HW)
    assert np.array_equal(got(nhwc), bits32(w))
    back = fresh(B, C, HW)
    util.guarded_call('nhwc_to_nchw_f32', nhwc, back, B, C, HW)
    assert np.array_equal(got(back), bits)
    w = np.zeros((B, C, HW), np.float32)
    twin('nhwc_to_nchw_f32', rc.nchw_to_nhwc(bits).view(np.float32), w, B, C, HW)
    assert np.array_equal(got(back), bits32(w))
    for Cpad in rc.layout_pads(C):
        pad = fresh(B, HW, Cpad)
        util.guarded_call('nchw_to_nhwc_pad_f32', src, pad, B, C, HW, Cpad)
        assert np.array_equal(got(pad), rc.nchw_to_nhwc_pad(bits, Cpad)), f'Cpad={Cpad}'
        w = np.zeros((B, HW, Cpad), np.float32)
        twin('nchw_to_nhwc_pad_f32', bits.view(np.float32), w, B, C, HW, Cpad)
        assert np.array_equal(got(pad), bits32(w)), f'Cpad={Cpad} (twin)'


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flav', ['f16', 'bf16'])
@pytest.mark.parametrize('n', rc.CAST_NS)
def test_casts(flav, n):
    """both directions bit for bit against torch's CPU cast (round to nearest even) on the type's rounding edges; of a NaN only NaN-ness"""
    dt = rc.torch_dtype(flav)
    x = rc.build_cast_to16(flav, n)
    out = torch.full((n,), 0x5A5A, dtype=torch.int16, device='cuda')
    util.guarded_call(f'cast_f32_to_{flav}', torch.from_numpy(x).cuda(), out.view(dt), n)
    got, want = out.cpu().numpy().view(np.uint16), rc.cast_to16(flav, x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan]), [(float(v), hex(g), hex(w)) for v, g, w in zip(x[~nan], got[~nan], want[~nan]) if g != w][:8]
    assert np.isnan(rc.cast_from16(flav, got[nan])).all()
    b16 = rc.build_cast_from16(flav, n)
    out32 = torch.full((n,), SENTINEL, dtype=torch.int32, device='cuda')
    util.guarded_call(f'cast_{flav}_to_f32', torch.from_numpy(b16.view(np.int16)).cuda().view(dt), out32.view(torch.float32), n)
    got, want = out32.cpu().numpy().view(np.uint32), bits32(rc.cast_from16(flav, b16))
    nan = np.isnan(rc.cast_from16(flav, b16))
    assert np.array_equal(got[~nan], want[~nan]), [(hex(v), hex(g), hex(w)) for v, g, w in zip(b16[~nan], got[~nan], want[~nan]) if g != w][:8]
    assert np.isnan(got[nan].view(np.float32)).all()


@pytest.mark.parametrize('flav', ['f16', 'bf16'])
def test_casts_refuse(flav):
    """n % 4 != 0 and a pointer off its 16 bytes: VARHIP_EINVAL, output untouched"""
    dt = rc.torch_dtype(flav)
    x32 = torch.ones(16, device='cuda')
    x16 = torch.ones(16, dtype=dt, device='cuda')
    o16 = torch.full((16,), 0x5A5A, dtype=torch.int16, device='cuda')
    o32 = torch.full((16,), SENTINEL, dtype=torch.int32, device='cuda')
    for n, si, so in ((6, 0, 0), (8, 1, 0), (8, 0, 1)):
        refused(f'cast_f32_to_{flav}', [x32[si:], o16.view(dt)[so:], n])
        refused(f'cast_{flav}_to_f32', [x16[si:], o32.view(torch.float32)[so:], n])
    assert bool((o16 == 0x5A5A).all()) and bool((o32 == SENTINEL).all())
