"""The 16-bit attention kernel (var_amd/csrc/attn16.hip, varhip_attn_cached_f16 / _bf16) on a real MI355X over the two decks of
tests/attn16cases.py (proven on the CPU by tests/test_attn16_dispatch_cpu.py), every operand in a guard arena (tests/util.py), rows
[curL, Lmax) of K and V NaN, `out` NaN before the launch.

The selector deck: the softmax is exactly one-hot, so `out` must equal the selected V rows bit for bit in both flavours; a second launch on the
same buffers must repeat the bits; varhip_attn16_last_waves() must name the NW the case states.  The bar deck: `out` within the derived bar of
the float64 reference, elementwise (max err / bar printed per case, not a threshold), on score profiles that steer the running maximum."""
import numpy as np
import pytest

from tests import attn16cases as ac
from tests import util
from tests.test_kernels_gpu import _setup
from var_amd import abi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DT = {'f16': torch.float16, 'bf16': torch.bfloat16}


def launch(flav, b, twice=False):
    """varhip_attn_cached_<flav> on device copies of the case's operands -> (out [B2 l][H 64] of the 16-bit type on the host, NW of the launch);
    twice: a second launch on the same device buffers must write the same bits"""
    _, hip = _setup()
    c = b.case
    q, k, v = (torch.from_numpy(np.ascontiguousarray(a)).to(DT[flav]).cuda() for a in (b.q, b.k, b.v))
    for t, a in ((q, b.q), (k, b.k), (v, b.v)):
        assert np.array_equal(t.float().cpu().numpy(), a, equal_nan=True), 'the operands are not values of the type'
    out = torch.full((c['B2'] * c['l'], c['H'] * 64), float('nan'), dtype=DT[flav], device='cuda')
    name = 'attn_cached_' + flav
    util.guarded_call(name, q, k, v, out, c['B2'], c['l'], c['H'], c['curL'], c['Lmax'])
    nw = hip.lib().so.varhip_attn16_last_waves()
    if twice:
        first = out.clone()
        util.guarded_call(name, q, k, v, out, c['B2'], c['l'], c['H'], c['curL'], c['Lmax'])
        bad = (first.view(torch.int16) != out.view(torch.int16)).nonzero()
        assert bad.numel() == 0, f"{c['name']} {flav}: a second launch differs, first at {tuple(bad[0].tolist())}"
    return out.cpu(), nw


@pytest.mark.parametrize('flav', ac.FLAVOURS)
@pytest.mark.parametrize('case', ac.sel_cases(), ids=lambda c: c['name'])
def test_selector_deck_returns_the_selected_rows_exactly(case, flav):
    b = ac.build_selector(case)
    out, nw = launch(flav, b, twice=True)
    assert nw == case['nw'], f"{case['name']} {flav}: varhip_attn16_last_waves() = {nw}, the deck states {case['nw']}"
    want = torch.from_numpy(b.expected).to(DT[flav])
    if not torch.equal(out, want):
        r, col = (out.float() != want.float()).nonzero()[0].tolist()             # (NaN != anything: an unwritten or poisoned element counts)
        bb, t, h, ch = r // case['l'], r % case['l'], col // 64, col % 64
        got = float(out[r, col])
        keys = np.flatnonzero(b.v[bb, h, :case['curL'], ch] == got)[:8].tolist()
        pytest.fail(f"{case['name']} {flav}: {int((out.float() != want.float()).sum())}/{out.numel()} elements differ, first at row {r} column {col} "
                    f"(b={bb} t={t} h={h} channel={ch}): got {got!r}, want {float(want[r, col])!r} = v[key {int(b.sel[bb, h, t])}]; keys of this slice "
                    f"that hold the value got at this channel: {keys}")


def test_every_wave_count_is_launched_and_reported():
    """one launch per l of the selector deck (one slice, curL = l): the hook reports the restated choice, and the deck reaches NW = 1, 2, 3, 4"""
    seen = {}
    for flav in ac.FLAVOURS:
        for l in sorted({c['l'] for c in ac.sel_cases()}):
            c = dict(name=f'waves l={l}', l=l, curL=l, Lmax=l + 33, B2=1, H=1, nw=ac.waves(l))
            b = ac.build_selector(c)
            out, nw = launch(flav, b)
            assert nw == ac.waves(l), f'{flav} l={l}: varhip_attn16_last_waves() = {nw}, restated choice {ac.waves(l)}'
            assert torch.equal(out, torch.from_numpy(b.expected).to(DT[flav])), f'{flav} l={l}'
            seen[l] = nw
    print('l -> NW:', seen)
    assert set(seen.values()) == {1, 2, 3, 4}


@pytest.mark.parametrize('flav', ac.FLAVOURS)
@pytest.mark.parametrize('case', ac.bar_cases(), ids=lambda c: c['name'])
def test_bar_deck_within_the_derived_bar(case, flav):
    b = ac.build_bar(case, flav)
    ref, bar = ac.reference(b)
    out, nw = launch(flav, b, twice=True)
    assert nw == case['nw'], f"{case['name']} {flav}: varhip_attn16_last_waves() = {nw}, the deck states {case['nw']}"
    ac.within(f"{case['name']} {flav}", out.float().numpy(), ref, bar)


@pytest.mark.parametrize('flav', ac.FLAVOURS)
def test_a_refused_call_leaves_the_hook(flav):
    """curL > Lmax: VARHIP_EINVAL, nothing written, varhip_attn16_last_waves() still names the launch before (l = 97: NW = 4; the refused l = 1 would be 1)"""
    _, hip = _setup()
    so = hip.lib().so
    _, nw = launch(flav, ac.build_selector(dict(name='before', l=97, curL=97, Lmax=97, B2=1, H=1, nw=4)))
    assert nw == 4 and so.varhip_attn16_last_waves() == 4
    q, k, v, out = (torch.full(s, float('nan'), dtype=DT[flav], device='cuda') for s in ((1, 64), (1, 1, 8, 64), (1, 1, 8, 64), (1, 64)))
    name = 'attn_cached_' + flav
    rc = util.guarded_invoke(f'varhip_{name}', [q, k, v, out, 1, 1, 1, 9, 8], lambda *a: hip.lib().fn[name](*a, hip.current_stream()), torch.cuda.synchronize)
    assert rc == abi.EINVAL and so.varhip_attn16_last_waves() == 4 and bool(torch.isnan(out).all())
