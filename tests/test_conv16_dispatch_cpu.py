"""tests/conv16cases.py validated without a GPU: the table reaches what it claims (pick_conv16 and the instantiation choice of dispatch_conv16,
var_amd/csrc/conv16.hip, restated here on their own), every expected varhip_conv16_last_pick value is what that restatement gives, the dyadic
operands keep every partial sum exact in fp32, exercise the final rounding and stay off the clamp, and the data can see the faults a
convolution kernel is prone to: each planted fault changes the expected output of every case it applies to.
tests/test_conv16_dispatch_gpu.py then runs the same table through the HIP library."""
import pytest

torch = pytest.importorskip('torch')

from tests import conv16cases as cc          # noqa: E402

F = torch.nn.functional


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch, restated from conv16.hip
def geometry(c):
    """-> (M, Hm, Wm, phase, nz): the pixels and the map the kernel works on"""
    if c['entry'] == 'upconv':
        return c['B'] * (c['H'] // 2) * (c['W'] // 2), c['H'] // 2, c['W'] // 2, 1, 4
    return c['B'] * c['H'] * c['W'], c['H'], c['W'], 0, 1


def pick_conv16(c):
    M, Hm, Wm, phase, nz = geometry(c)
    N, force = c['Cout'], c['wm']
    bn = 160 if N % 160 == 0 else 128
    if (not phase and c['omode'] == 0 and force not in (2, 4) and (N % 160 == 0 or N % 128 == 0) and Hm * Wm * c['Cin'] * 2 < 2 ** 31
            and (force == 8 or (M // 256) * (N // bn) >= 256)):
        if Wm % 32 == 0 and Hm % 8 == 0:
            return 1
        if Wm % 16 == 0 and Hm % 16 == 0:
            return 2
    big_wgs = ((M + 255) // 256) * ((N + 159) // 160) * nz
    return 3 if (force == 4 if force else big_wgs >= 256) else 0


def conv16h_lds(tnw, pw, gn_cin):
    npiece = ((256 // pw + 2) * (pw + 2) + 15) // 16
    return 2 * npiece * 1024 + 3 * tnw * 32 * 64 + npiece * 64 + gn_cin * 8


def instantiation(c):
    """-> (kernel digit, TNW, GN, nz) of the instantiation dispatch_conv16 launches, None where the call is refused"""
    pick = pick_conv16(c)
    N, nz = c['Cout'], geometry(c)[4]
    gn = int(c['entry'] == 'gnconv')
    if pick in (1, 2):
        tnw = 5 if N % 160 == 0 else 4
        if gn and conv16h_lds(tnw, 32 if pick == 1 else 16, c['Cin']) > 80 * 1024:
            return None
        return pick, tnw, gn, nz
    if gn:
        return None
    if N % 160 == 0:
        return pick, 5, 0, nz
    if N % 128 == 0:
        return pick, 4, 0, nz
    return 0, (2 if N % 64 == 0 else 1), 0, nz


HALO = [(k, t, g, 1) for k in (1, 2) for t in (5, 4) for g in (0, 1)]
TILE = [(3, 5, 0), (0, 5, 0), (3, 4, 0), (0, 4, 0), (0, 2, 0), (0, 1, 0)]


def test_every_expected_hook_value_is_the_restated_dispatch():
    for c in cc.cases():
        inst = instantiation(c)
        if c['einval']:
            assert inst is None and c['expect'] is None, cc.name(c)
        else:
            assert inst is not None and c['expect'] == cc.hook(inst[0], inst[1], inst[2], inst[3]), f'{cc.name(c)}: the restated dispatch gives {inst}'
        if c['wm'] == 0:
            assert c['group'] == 'auto'


def test_table_covers_every_instantiation_and_path():
    assert len(HALO) + len(TILE) == 14
    for flav in cc.FLAVOURS:
        mine = [c for c in cc.cases(flav=flav) if not c['einval']]
        forced = [c for c in mine if c['wm']]
        by = {}
        for c in forced:
            by.setdefault((c['entry'],) + instantiation(c), []).append(c)
        # the halo-patch kernel: 8 instantiations, each with one, two and three channel tiles, workgroup counts that deal evenly to the 8 XCDs and
        # counts that do not with at least one full round (q >= 1, rem != 0), 1, 2, 3 and 5 chunks, and a residual on some
        for inst in HALO:
            got = by.get((('gnconv' if inst[2] else 'conv'),) + inst, [])
            assert got, (flav, inst)
            ph, pw = (8, 32) if inst[0] == 1 else (16, 16)
            bn = 32 * inst[1]
            wgs = [(c['B'] * (c['H'] // ph) * (c['W'] // pw)) * (c['Cout'] // bn) for c in got]
            assert {1, 2, 3} <= {c['Cout'] // bn for c in got}, (flav, inst)
            assert any(w & 7 == 0 for w in wgs) and any(w & 7 and w >> 3 for w in wgs) and any(w < 8 for w in wgs), (flav, inst, wgs)
            assert {1, 2, 3, 5} <= {c['Cin'] // 32 for c in got}, (flav, inst)
            assert {0, 1} == {c['res'] for c in got}, (flav, inst)
            if pw == 16:
                assert any(c['W'] % 32 and (c['W'] // 16) % 2 for c in got), 'the 16 x 16 form by geometry, an odd number of patches per row'
            else:
                assert any(c['W'] % 16 == 0 and c['H'] % 16 == 0 for c in got), 'a map both patch forms take: 8 x 32 must win'
        # k_conv16: 6 instantiations, plain and in the phase form
        for kern, tnw, _ in TILE:
            bm = 256 if kern == 3 else 128
            plain, phase = by.get(('conv', kern, tnw, 0, 1), []), by.get(('upconv', kern, tnw, 0, 4), [])
            assert plain and phase, (flav, kern, tnw)
            for got in (plain, phase):
                M = [geometry(c)[0] for c in got]
                hw = [geometry(c)[1] * geometry(c)[2] for c in got]
                assert any(m % 256 == 0 for m in M) and any(m % bm for m in M), (flav, kern, tnw)
                assert any(h < 128 and c['B'] > 1 for h, c in zip(hw, got)), 'several images inside one pixel tile'
            assert {0, 1} == {c['res'] for c in plain}
            assert any(c['H'] * c['W'] < 128 and c['B'] == 1 for c in plain) and any(c['H'] * c['W'] < 128 and c['B'] >= 3 for c in plain)
            assert any(c['B'] > 1 and c['H'] * c['W'] > 128 and (c['H'] * c['W']) % 128 for c in plain), 'an image boundary and a tile boundary that do not coincide'
            if tnw >= 4:
                assert {1, 2} <= {c['Cout'] // (32 * tnw) for c in plain}, 'a second channel tile'
            if tnw == 4:
                assert any(c['Cout'] // 128 == 3 for c in plain)
            if tnw == 2:
                assert {1, 3} <= {c['Cout'] // 64 for c in plain}
        # the two epilogues of k_conv16<1, ..>: vector (Cout % 4 == 0, out_mode 0) with a partial last channel tile, element-wise with the 16-bit
        # NHWC store (with and without a residual) and with both fp32 NCHW stores
        t1 = by[('conv', 0, 1, 0, 1)]
        assert any(c['Cout'] % 4 == 0 and c['Cout'] % 32 and c['Cout'] > 32 and c['omode'] == 0 for c in t1)
        assert any(c['Cout'] % 4 == 0 and c['Cout'] % 32 and c['omode'] == 0 for c in by[('upconv', 0, 1, 0, 4)])
        for res in (0, 1):
            assert any(c['Cout'] % 4 and c['omode'] == 0 and c['res'] == res and c['Cout'] > 4 for c in t1)
        for omode in (1, 2):
            assert {3, 4, 8} <= {c['Cout'] for c in t1 if c['omode'] == omode}
        assert {2, 4} <= {c['wm'] for c in t1 if c['omode']}
        # the automatic picker: each threshold from both sides, one step of B apart
        auto = [c for c in mine if c['wm'] == 0]
        M = lambda c: geometry(c)[0]
        halo_side = sorted((M(c) // 256) * (c['Cout'] // 160) for c in auto if c['entry'] == 'conv' and c['W'] % 32 == 0)
        assert halo_side == [255, 256]
        for entry in ('conv', 'upconv'):
            big_side = sorted(-(-M(c) // 256) * -(-c['Cout'] // 160) * geometry(c)[4] for c in auto if c['entry'] == entry and (entry == 'upconv' or c['W'] % 16))
            assert big_side[0] < 256 <= big_side[1] and big_side[1] - big_side[0] <= 4, big_side
        assert {instantiation(c)[0] for c in auto} == {0, 1, 3}
    assert [c for c in cc.cases() if c['einval'] and c['Cin'] == 640 and c['W'] % 32 == 0 and c['H'] % 8 == 0]


def _unique(entries):
    seen, out = set(), []
    for c in cc.cases(flav='f16'):
        key = (c['entry'], c['B'], c['H'], c['W'], c['Cin'], c['Cout'], c['res'], c['omode'])
        if c['entry'] in entries and key not in seen:
            seen.add(key); out.append(c)
    return out


@pytest.mark.parametrize('group', ['halo', 'tile', 'omode', 'phase', 'auto'])
def test_operands_are_exact_and_exercise_the_rounding(group):
    """the three conditions on the dyadic operands, on the reference alone: every partial sum below 2^24 grid units; in the 16-bit stores at least a
    quarter of the exact results cannot be held by the output type (both flavours); in the fp32 stores at most half sit on the clamp"""
    for c in _unique(('conv', 'upconv')):
        if c['group'] != group:
            continue
        o = cc.operands(c)
        assert cc.exactness_budget(c, o) < 2 ** 24, cc.name(c)
        for t in (o.x, o.wnum, o.wexp, o.bias / cc.BIAS_GRID, o.bias / o.grid, o.w / o.grid) + ((o.resid * 16.0,) if o.resid is not None else ()):
            assert torch.equal(t, t.round()), cc.name(c)
        assert float(o.x.abs().max()) <= 2 and float(o.wnum.abs().max()) <= 2 and torch.equal(o.w, o.wnum * torch.pow(2.0, -o.wexp))
        assert torch.equal(o.w.to(torch.bfloat16).double(), o.w) and torch.equal(o.w.half().double(), o.w) and torch.equal(o.x.to(torch.bfloat16).double(), o.x)
        if o.resid is not None:
            assert torch.equal(o.resid.to(torch.bfloat16).double(), o.resid) and torch.equal(o.resid.half().double(), o.resid)
        v = cc.conv64(c, o.x, o.w) + o.bias
        if o.resid is not None:
            v = v + o.resid
        if c['omode'] == 0:
            for flav in cc.FLAVOURS:
                share = cc.needs_rounding(v, flav)
                assert share >= 0.25, f'{cc.name(c)}: only {share:.2f} of the exact results need the {flav} rounding'
                cc.expected(dict(c, flav=flav), o)                       # (asserts that the cast rounds once)
            assert (o.bias / cc.BIAS_GRID % 2 == 1).any(), 'no bias uses the last bit of its grid'
        else:
            share = float((v.abs() >= 1.0).double().mean())
            assert share <= 0.5, f'{cc.name(c)}: {share:.2f} of the results sit on the clamp'
            assert bool((v >= 1.0).any()) and bool((v <= -1.0).any()), f'{cc.name(c)}: the clamp is never reached'
            want = cc.expected(dict(c, flav='f16'), o)
            assert not bool((want == cc.SENTINEL32).any()) and torch.equal(want, cc.expected(dict(c, flav='bf16'), o))


# ---------------------------------------------------------------------------------------------------------------------
# planted faults: a wrong kernel's output, computed here, must differ from the expectation on the case's own data
FAULTS = ('tap', 'replicate', 'swap_hw', 'prev_image', 'bias_late', 'resid_late', 'dup_tile')


def applies(c, fault):
    """resid_late needs a residual; dup_tile a second channel.  Everything else applies to every plain case (bias_late: behind the rounding of the
    16-bit stores, behind the clamp of the fp32 ones, which round nothing)."""
    return (fault != 'resid_late' or c['res']) and (fault != 'dup_tile' or c['Cout'] > 1)


def planted(c, o, fault, good):
    B, H, W, Cout, flav = c['B'], c['H'], c['W'], c['Cout'], c['flav']
    xn = o.x.permute(0, 3, 1, 2)
    if fault == 'tap':                                         # tap (ky 0, kx 2) reads one pixel to the left of its place
        xp = F.pad(xn, (1, 1, 1, 1))
        delta = torch.einsum('bchw,oc->bhwo', xp[:, :, 0:H, 1:W + 1] - xp[:, :, 0:H, 2:W + 2], o.w[:, 0, 2, :])
        return cc.finish(c, flav, cc.conv64(c, o.x, o.w) + delta, o.bias, o.resid)
    if fault == 'replicate':                                   # the border repeats the edge pixel instead of zeros
        return cc.finish(c, flav, cc.conv64(c, o.x, o.w, padded=F.pad(xn, (1, 1, 1, 1), mode='replicate')), o.bias, o.resid)
    if fault == 'swap_hw':                                     # pixel (y, x) taken at x * H + y: the map read as W rows of H (a transposed map where H == W)
        if H != W:
            acc = cc.conv64(c, o.x.reshape(B, W, H, -1), o.w).reshape(B, H, W, Cout)
        else:
            acc = cc.conv64(c, o.x.transpose(1, 2), o.w)
        return cc.finish(c, flav, acc, o.bias, o.resid)
    if fault == 'prev_image':                                  # the halo row above an image is the last row of the image before it (the first wraps to the last)
        xp = F.pad(xn, (1, 1, 1, 1)).clone()
        xp[:, :, 0, 1:-1] = xn.roll(1, 0)[:, :, H - 1, :]
        return cc.finish(c, flav, cc.conv64(c, o.x, o.w, padded=xp), o.bias, o.resid)
    acc = cc.conv64(c, o.x, o.w)
    if fault == 'bias_late':
        if c['omode'] == 0:
            early = cc.round16(acc + (o.resid if o.resid is not None else 0.0), flav, exact=False).double()
            return cc.round16(early + o.bias, flav, exact=False)
        v = acc.clamp(-1.0, 1.0) + o.bias
        return ((v + 1.0) * 0.5 if c['omode'] == 1 else v).float().permute(0, 3, 1, 2).contiguous()
    if fault == 'resid_late':
        return cc.round16(cc.round16(acc + o.bias, flav, exact=False).double() + o.resid, flav, exact=False)
    if fault == 'dup_tile':                                    # a channel tile (a wave's half of it, a lane's four channels, a channel) stored over its neighbour as well
        bn = 32 * ((c['expect'] // 10) % 10)
        wd = next(w for w in (bn, bn // 2, 4, 1) if w < Cout)
        out = good.clone()
        n = min(wd, Cout - wd)
        if c['omode'] == 0:
            out[..., wd:wd + n] = good[..., :n]
        else:
            out[:, wd:wd + n] = good[:, :n]
        return out
    raise KeyError(fault)


@pytest.mark.parametrize('group', ['halo', 'tile', 'omode', 'auto'])
def test_the_data_sees_every_planted_fault(group):
    ran = {f: 0 for f in FAULTS}
    for c0 in _unique(('conv',)):
        if c0['group'] != group:
            continue
        o = cc.operands(c0)
        for flav in cc.FLAVOURS:
            c = dict(c0, flav=flav)
            good = cc.expected(c, o)
            for fault in FAULTS:
                if not applies(c, fault):
                    continue
                assert not torch.equal(planted(c, o, fault, good), good), f'{cc.name(c)}: the expectation is blind to the planted fault {fault!r}'
                ran[fault] += 1
    assert all(n > 0 for f, n in ran.items() if not (f == 'resid_late' and group == 'omode')), ran
