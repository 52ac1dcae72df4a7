"""The fp32 attention kernel (var_amd/csrc/attn.hip, varhip_attn_cached_f32) on a real MI355X over the decks of tests/attncases.py (proven on the
CPU by tests/test_attn_dispatch_cpu.py), every operand in a guard arena (tests/util.py), rows [curL, Lmax) of K and V NaN, `out` NaN before
every launch.

The selector deck: the softmax is one-hot up to a stray mass far below half an ulp, so `out` must equal the selected V rows bit for bit, and
varhip_attn_last_waves() must name the NW the case states.  The bar deck: `out` within the derived bar of the float64 reference, elementwise
(max err / bar printed per case, not a threshold), and still bit-equal to the oracle's twin.  The forced-NW deck: every NW of 1 .. 4 on shapes
where that leaves 0 to 3 waves without queries, bit-identical to the dispatch's own launch and within the bar."""
import numpy as np
import pytest

from tests import attncases as ac
from tests import util
from tests.test_kernels_gpu import _setup
from var_amd import abi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

NAME = 'attn_cached_f32'


def device_operands(b):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (b.q, b.k, b.v))


def launch(c, q, k, v):
    """varhip_attn_cached_f32 on the device operands into a fresh NaN-filled out -> (out [B2 l][H 64] on the host, NW of the launch)"""
    _, hip = _setup()
    out = torch.full((c['B2'] * c['l'], c['H'] * 64), float('nan'), dtype=torch.float32, device='cuda')
    util.guarded_call(NAME, q, k, v, out, c['B2'], c['l'], c['H'], c['curL'], c['Lmax'])
    return out.cpu(), hip.lib().so.varhip_attn_last_waves()


@pytest.fixture(autouse=True)
def dispatch_decides():
    """every test starts and ends with the hook at 0"""
    _, hip = _setup()
    hip.lib().so.varhip_attn_force_waves(0)
    yield
    hip.lib().so.varhip_attn_force_waves(0)


@pytest.mark.parametrize('case', ac.sel_cases(), ids=lambda c: c['name'])
def test_selector_deck_returns_the_selected_rows_exactly(case):
    b = ac.build_selector(case)
    out, nw = launch(case, *device_operands(b))
    assert nw == ac.waves(case['l']) == case['nw'], f"{case['name']}: varhip_attn_last_waves() = {nw}, the restated dispatch says {ac.waves(case['l'])}"
    want = torch.from_numpy(b.expected)
    if not torch.equal(out, want):
        r, col = (out != want).nonzero()[0].tolist()                            # (NaN != anything: an unwritten or poisoned element counts)
        bb, t, h, ch = r // case['l'], r % case['l'], col // 64, col % 64
        got = float(out[r, col])
        keys = np.flatnonzero(b.v[bb, h, :case['curL'], ch] == got)[:8].tolist()
        pytest.fail(f"{case['name']}: {int((out != want).sum())}/{out.numel()} elements differ, first at row {r} column {col} "
                    f"(b={bb} t={t} h={h} channel={ch}): got {got!r}, want {float(want[r, col])!r} = v[key {int(b.sel[bb, h, t])}]; keys of this slice "
                    f"that hold the value got at this channel: {keys}")


@pytest.mark.parametrize('case', ac.bar_cases(), ids=lambda c: c['name'])
def test_bar_deck_within_the_derived_bar_and_equal_to_the_twin(case):
    L, _ = _setup()
    b, ref, bar = ac.bar_built(case)
    out, nw = launch(case, *device_operands(b))
    assert nw == case['nw'], f"{case['name']}: varhip_attn_last_waves() = {nw}, the deck states {case['nw']}"
    ac.within(case['name'], out.numpy(), ref, bar)
    want = torch.from_numpy(ac.twin(L, b))                                      # the existing contract is kept, not replaced
    bad = (out.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert bad.numel() == 0, f"{case['name']}: {bad.shape[0]} elements differ from varref_attn_cached_f32, first at {tuple(bad[0].tolist())}"


@pytest.mark.parametrize('nw', (1, 2, 3, 4))
@pytest.mark.parametrize('case', ac.forced_cases(), ids=lambda c: c['name'])
def test_forced_wave_count_computes_the_same_bits(case, nw):
    """A query's arithmetic depends only on its own wave's 32 queries (the __any that skips a rescale whose alpha is 1.0 for all of them: same bits
    either way) and on the tile walk, never on NW: NW decides which waves share a workgroup's K/V stages, how the staging work is split among them,
    and how many waves of the last workgroup have no query (ac.forced_idle(l, nw): they only stage and sync).  So a forced launch must write the
    bits of the dispatch's own"""
    _, hip = _setup()
    so = hip.lib().so
    b, ref, bar = ac.bar_built(case)
    ops = device_operands(b)
    own, own_nw = launch(case, *ops)
    assert own_nw == ac.waves(case['l'])
    try:
        so.varhip_attn_force_waves(nw)
        out, got_nw = launch(case, *ops)
    finally:
        so.varhip_attn_force_waves(0)
    assert got_nw == nw, f"{case['name']}: forced NW = {nw}, varhip_attn_last_waves() = {got_nw}"
    print(f"{case['name']} NW = {nw}: {ac.forced_idle(case['l'], nw)} waves without queries")
    ac.within(f"{case['name']} NW = {nw}", out.numpy(), ref, bar)
    bad = (out.view(torch.int32) != own.view(torch.int32)).nonzero()
    assert bad.numel() == 0, f"{case['name']}: NW = {nw} differs from NW = {own_nw} in {bad.shape[0]} elements, first at {tuple(bad[0].tolist())}"
    _, back = launch(case, *ops)
    assert back == ac.waves(case['l']), 'the hook at 0 gives the choice back to the dispatch'


def test_the_hook_takes_1_to_4_and_nothing_else():
    _, hip = _setup()
    so = hip.lib().so
    c = dict(name='hook', l=33, curL=33, Lmax=40, B2=1, H=1, nw=2)
    b = ac.build_selector(c)
    ops = device_operands(b)
    try:
        for req in (-1, 5, 64, 0):
            so.varhip_attn_force_waves(3)
            so.varhip_attn_force_waves(req)
            out, nw = launch(c, *ops)
            assert nw == 2, f'varhip_attn_force_waves({req}) is not the same as 0: NW = {nw}'
            assert torch.equal(out, torch.from_numpy(b.expected))
    finally:
        so.varhip_attn_force_waves(0)


def test_a_second_launch_repeats_the_bits():
    """l = 97, curL = 129, B2 = 2, H = 3 (NW = 4, five tiles, one key in the last), twice into fresh NaN outputs: the epilogue's O transpose aliases the
    K/V stages in LDS, so a read ahead of the last barrier shows up as a difference"""
    c = dict(name='asc l=97 curL=129 twice', kind='asc', l=97, curL=129, Lmax=162, B2=2, H=3, nw=4, sibling=None, X=None)
    b, ref, bar = ac.bar_built(c)
    ops = device_operands(b)
    first, nw = launch(c, *ops)
    second, _ = launch(c, *ops)
    assert nw == 4
    ac.within(c['name'], first.numpy(), ref, bar)
    bad = (first.view(torch.int32) != second.view(torch.int32)).nonzero()
    assert bad.numel() == 0, f'a second launch differs in {bad.shape[0]} elements, first at {tuple(bad[0].tolist())}'


@pytest.mark.parametrize('what, B2, l, H, curL, Lmax', [('curL > Lmax', 1, 1, 1, 9, 8), ('l = 0', 1, 0, 1, 8, 8), ('B2 = 65536', 65536, 1, 1, 8, 8)])
def test_a_refused_call_writes_nothing(what, B2, l, H, curL, Lmax):
    """VARHIP_EINVAL, `out` still NaN, varhip_attn_last_waves() still names the launch before (l = 97: NW = 4; the refused calls would be 1).  The
    operands are sized for B2 = 1, l = 1: a refused call reads none of them"""
    _, hip = _setup()
    so = hip.lib().so
    before = dict(name='before', l=97, curL=97, Lmax=97, B2=1, H=1, nw=4)
    _, nw = launch(before, *device_operands(ac.build_selector(before)))
    assert nw == 4
    q, k, v, out = (torch.full(s, float('nan'), dtype=torch.float32, device='cuda') for s in ((1, 64), (1, 1, 8, 64), (1, 1, 8, 64), (1, 64)))
    rc = util.guarded_invoke(f'varhip_{NAME}', [q, k, v, out, B2, l, H, curL, Lmax], lambda *a: hip.lib().fn[NAME](*a, hip.current_stream()), torch.cuda.synchronize)
    assert rc == abi.EINVAL, f'{what}: rc = {rc}'
    assert so.varhip_attn_last_waves() == 4 and bool(torch.isnan(out).all())
