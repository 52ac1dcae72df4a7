"""The 16-bit mode's pieces that run on every 16-bit step, each as a unit on a real MI355X, in both flavours (f16, bf16): the AdaLN block
composite (varhip_adaln_block_*), the batched GEMM (varhip_gemm_nt_* with batch > 1: the products of the VAE's attention) and the VAE
AttnBlock (the 16-bit op set's attnblock: DecoderEngine.ops16(flavour).attnblock).  LayerNorm + modulate with a 16-bit output is pinned in test_kernels_gpu.test_ln_modulate_exact.

Every tolerance is stated from the rounding points of the computation it checks:
  ACC  the fp32 accumulation of a product in another order than the reference's: at most 2e-6 * sum_k |a_k||w_k| (K <= 9216);
  U    one rounding to the 16-bit type: at most U * |value|, U = 2^-11 (fp16) or 2^-8 (bfloat16), the unit roundoff; where two computations
       round values that differ by d, the rounded values differ by at most d + one ulp of the result.
Every check prints its largest error / bar ratio.
"""
import math

import numpy as np
import pytest

from tests import util
from tests.test_f16_gpu import _models

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ACC = 2e-6
FLAV = {'f16': (torch.float16, 2.0 ** -11), 'bf16': (torch.bfloat16, 2.0 ** -8)}
EPI_GELU, EPI_RESID = 1, 2


def _hip():
    from var_amd import hip
    return hip


def _ulp(v, fl):
    """one unit in the last place of 16-bit values v (as float64): 2^(e - 11) for fp16, 2^(e - 8) for bfloat16, |v| in [2^(e-1), 2^e)"""
    _, e = torch.frexp(v)
    bits, emin = (11, -13) if fl == 'f16' else (8, -125)
    e = torch.where(v == 0, torch.full_like(e, emin), e.clamp_min(emin))
    return torch.pow(2.0, (e - bits).double())


def _ratio(name, err, bar):
    r = float((err / bar).max())
    print(f'{name}: max |err| {float(err.max()):.3e}, max err/bar {r:.3f}')
    assert r <= 1.0, f'{name}: {int((err > bar).sum())} of {err.numel()} elements beyond the bar (max err/bar {r:.3f})'


# ---------------------------------------------------------------------------------------------------------------------
BLOCK_CASES = [(4, 1, 16, 4096, 0, 680, 1), (4, 9, 16, 4096, 5, 680, 1), (2, 256, 16, 4096, 424, 680, 1), (2, 100, 30, 7680, 91, 680, 0),
               (2, 36, 36, 9216, 50, 2240, 1)]
PATCH_NUMS = {680: (1, 2, 3, 4, 5, 6, 8, 10, 13, 16), 2240: (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)}      # sum of pn^2 = Lmax


@pytest.mark.parametrize('fl', ['f16', 'bf16'])
@pytest.mark.parametrize('B2,l,H,hidden,pos0,Lmax,l2', BLOCK_CASES)
def test_adaln_block16(fl, B2, l, H, hidden, pos0, Lmax, l2):
    """varhip_adaln_block_{f16,bf16}: one AdaLNSelfAttn block at the d16 / d30 / d36 widths, the first scale, a small one and the last d16 scale.

    (a) The composite is DEFINED as the seven entry points block.hip lists, called one after another: the same bits in x, x2, the k / v cache
        and the 16-bit scratch (LN output, q, attention output, MLP hidden).  A fusion that changes the rounding replaces this with its own
        argument.
    (b) Against the CPU twin's block (OracleVAR.block, f16 = the flavour: fp32 arithmetic with the same rounding points) on the same inputs.
        The two differ only in the order of fp32 accumulation inside the products and attention (ACC), and in the 16-bit rounding flips that
        follow (where the two fp32 values straddle a rounding boundary the results differ by one ulp).  The LayerNorm outputs of the first
        step are identical (same fp32 code, test_ln_modulate_exact).
        Cache rows [pos0, pos0 + l), per element: one ulp of the twin's value + the difference before the rounding, d_qkv = ACC |xn1||Wqkv|^T
        carried through the L2 norm (d_khat = (d_k + |k| ||d_k|| / ||k||) / ||k||; q likewise times exp(sm)), or times 1/32 without it.
        x: a worst-case sum of one ulp for every element of every intermediate exceeds the signal, so the bar is root-sum-square: each
        rounding point contributes an independent difference of variance ulp^2 (a flip at every element: an upper bound), each accumulation one
        of standard deviation ACC sum |a||w|, fp32 element-wise steps 1e-6 |v|; variances are carried in float64 from the HIP run's own
        intermediates through q.K^T, the softmax (var(d_p) <= 2 p^2 (var(d_s) + sum p^2 var(d_s))), p.V, the gated residual x2 = x + g1 (.),
        the LayerNorm (var(d_xhat) <= 3 rstd^2 (var(d_x2) + mean var / C + xhat^2 mean(xhat^2 var) / C)), fc1 + GELU (|gelu'| <= 1.13) and
        x = x2 + g2 (.) (factor 2: x2's difference enters twice).  Bar = 8 sigma.
        Cache rows outside [pos0, pos0 + l) keep their sentinels."""
    hip = _hip()
    util.ensure_oracle_built()
    from oracle.var_oracle import OracleVAR
    dt = FLAV[fl][0]
    C, M = 64 * H, B2 * l
    g = torch.Generator().manual_seed(B2 * l + H + hidden)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x = rn(M, C)
    x[::5] += 30.0
    ada = rn(B2, 6 * C, sc=0.3) + 0.2
    wq = rn(3 * C, C, sc=C ** -0.5).to(dt)
    bq = torch.cat([rn(C, sc=0.1), torch.zeros(C), rn(C, sc=0.1)])                     # [q_bias, 0, v_bias] as the engine passes it
    sm = math.log(4.0) + rn(H, sc=0.5)
    sm[0] = 6.0                                                                         # beyond clamp_max(log 100)
    wp, bp = rn(C, C, sc=0.5 * C ** -0.5).to(dt), rn(C, sc=0.05)
    w1, b1 = rn(hidden, C, sc=C ** -0.5).to(dt), rn(hidden, sc=0.05)
    w2, b2 = rn(C, hidden, sc=0.5 * hidden ** -0.5).to(dt), rn(C, sc=0.05)
    kc, vc = rn(B2, H, Lmax, 64, sc=0.5), rn(B2, H, Lmax, 64)
    if l2:                                           # cached keys of earlier scales are unit vectors in the real loop
        kc = kc / kc.norm(dim=-1, keepdim=True)
    kc[:, :, pos0:] = 3.0; vc[:, :, pos0:] = -3.0    # sentinels: [pos0, pos0 + l) must be written, the rows after it must survive
    kc, vc = kc.to(dt), vc.to(dt)

    d = {k: v.cuda() for k, v in dict(ada=ada, wq=wq, bq=bq, sm=sm, wp=wp, bp=bp, w1=w1, b1=b1, w2=w2, b2=b2).items()}
    def fresh():
        return dict(x=x.cuda(), x2=torch.full((M, C), float('nan'), device='cuda'), xn=torch.zeros(M, C, dtype=dt, device='cuda'),
                    q=torch.zeros(M, C, dtype=dt, device='cuda'), att=torch.zeros(M, C, dtype=dt, device='cuda'),
                    hid=torch.zeros(M, hidden, dtype=dt, device='cuda'), kc=kc.cuda(), vc=vc.cuda())
    smp = d['sm'] if l2 else None
    A = fresh()
    util.guarded_call('adaln_block_' + fl, A['x'], A['x2'], A['xn'], A['q'], A['att'], A['hid'], d['ada'], 6 * C, d['wq'], d['bq'], smp, 0.03125, l2,
             d['wp'], d['bp'], d['w1'], d['b1'], d['w2'], d['b2'], A['kc'], A['vc'], B2, l, C, H, hidden, pos0, Lmax, 1e-6)
    S = fresh()
    g1, g2, s1, s2, h1, h2 = (d['ada'][:, i * C:] for i in range(6))
    ln, gemm = f'ln_modulate_{fl}out', 'gemm_nt_' + fl
    util.guarded_call(ln, S['x'], s1, 6 * C, h1, 6 * C, S['xn'], M, C, l, 1e-6)
    util.guarded_call('gemm_qkv_' + fl, S['xn'], C, d['wq'], C, d['bq'], M, C, C, smp, 0.03125, l2, S['q'], S['kc'], S['vc'], B2, l, H, pos0, Lmax)
    util.guarded_call('attn_cached_' + fl, S['q'], S['kc'], S['vc'], S['att'], B2, l, H, pos0 + l, Lmax)
    util.guarded_call(gemm, S['att'], C, d['wp'], C, d['bp'], S['x2'], C, 0, M, C, C, EPI_RESID, S['x'], C, 0, g1, 6 * C, l, 1, 0, 0, 0)
    util.guarded_call(ln, S['x2'], s2, 6 * C, h2, 6 * C, S['xn'], M, C, l, 1e-6)
    util.guarded_call(gemm, S['xn'], C, d['w1'], C, d['b1'], S['hid'], hidden, 1, M, hidden, C, EPI_GELU, None, 0, 0, None, 0, 1, 1, 0, 0, 0)
    util.guarded_call(gemm, S['hid'], hidden, d['w2'], hidden, d['b2'], S['x'], C, 0, M, C, hidden, EPI_RESID, S['x2'], C, 0, g2, 6 * C, l, 1, 0, 0, 0)
    xn1 = torch.empty(M, C, dtype=dt, device='cuda')
    util.guarded_call(ln, x.cuda(), s1, 6 * C, h1, 6 * C, xn1, M, C, l, 1e-6)
    torch.cuda.synchronize()
    for k in A:                                                                       # (a)
        assert torch.equal(A[k], S[k]), f'(a) {k}: composite and its seven steps differ in {int((A[k] != S[k]).sum())} elements'

    # (b) the twin: one block of a depth-1 model holding these weights
    f = lambda t: t.float().numpy()
    sd = {'pos_start': np.zeros((1, 1, C), np.float32), 'pos_1LC': np.zeros((1, Lmax, C), np.float32),
          'blocks.0.attn.mat_qkv.weight': f(wq), 'blocks.0.attn.q_bias': f(bq[:C]), 'blocks.0.attn.v_bias': f(bq[2 * C:]),
          'blocks.0.attn.scale_mul_1H11': f(sm).reshape(1, H, 1, 1), 'blocks.0.attn.proj.weight': f(wp), 'blocks.0.attn.proj.bias': f(bp),
          'blocks.0.ffn.fc1.weight': f(w1), 'blocks.0.ffn.fc1.bias': f(b1), 'blocks.0.ffn.fc2.weight': f(w2), 'blocks.0.ffn.fc2.bias': f(b2)}
    twin = OracleVAR(sd, {'quantize.embedding.weight': np.zeros((2, 4), np.float32)}, PATCH_NUMS[Lmax], 1, attn_l2_norm=bool(l2), f16=fl)
    tk, tv = f(kc), f(vc)
    tx = torch.from_numpy(twin.block(0, f(x), f(ada), tk, tv, pos0, l)).cuda().double()
    tk, tv = torch.from_numpy(tk).cuda().double(), torch.from_numpy(tv).cuda().double()

    D = lambda t: t.double()
    rows = lambda t: D(t).repeat_interleave(l, dim=0)
    T = pos0 + l
    qkv = D(xn1) @ D(d['wq']).T + D(d['bq'])
    dqkv = ACC * (D(xn1).abs() @ D(d['wq']).abs().T)
    (q_, k_, v_), (dq, dk, dv) = qkv.view(M, 3, H, 64).unbind(1), dqkv.view(M, 3, H, 64).unbind(1)
    if l2:
        smx = D(d['sm']).clamp_max(math.log(100)).exp().view(1, H, 1)
        nq, nk = q_.norm(dim=-1, keepdim=True), k_.norm(dim=-1, keepdim=True)
        dq = smx * (dq + q_.abs() * dq.norm(dim=-1, keepdim=True) / nq) / nq
        dk = (dk + k_.abs() * dk.norm(dim=-1, keepdim=True) / nk) / nk
    else:
        dq = 0.03125 * dq
    heads = lambda t: t.reshape(B2, l, H, 64).permute(0, 2, 1, 3)                     # [B2*l, (H, 64)] -> [B2, H, l, 64]
    newk, newv = A['kc'][:, :, pos0:T], A['vc'][:, :, pos0:T]
    _ratio(f'{fl} k cache rows vs twin', (D(newk) - tk[:, :, pos0:T]).abs(), _ulp(tk[:, :, pos0:T], fl) + heads(dk) + 1e-6 * D(newk).abs())
    _ratio(f'{fl} v cache rows vs twin', (D(newv) - tv[:, :, pos0:T]).abs(), _ulp(tv[:, :, pos0:T], fl) + heads(dv) + 1e-6 * D(newv).abs())
    for cache, sent in ((A['kc'], 3.0), (A['vc'], -3.0)):
        assert bool((cache[:, :, T:] == sent).all()), 'a cache row beyond pos0 + l was written'
        assert torch.equal(cache[:, :, :pos0], (kc if sent > 0 else vc)[:, :, :pos0].cuda()), 'a cache row before pos0 was written'

    # x: root-sum-square of the differences (variances), see the docstring
    sq = lambda t: t * t
    q16, K, V = heads(D(A['q'])), D(A['kc'][:, :, :T]), D(A['vc'][:, :, :T])
    vQ = sq(heads(dq.reshape(M, C))) + sq(_ulp(q16, fl))
    vK, vV = torch.zeros_like(K), torch.zeros_like(V)
    vK[:, :, pos0:] = sq(heads(dk)) + sq(_ulp(K[:, :, pos0:], fl))
    vV[:, :, pos0:] = sq(heads(dv)) + sq(_ulp(V[:, :, pos0:], fl))
    Kt = K.transpose(-1, -2)
    s = q16 @ Kt
    vs = vQ @ sq(Kt) + sq(q16) @ vK.transpose(-1, -2) + sq(ACC * (q16.abs() @ Kt.abs())) + sq(1e-6 * s)
    p = torch.softmax(s, dim=-1)
    vp = 2 * sq(p) * (vs + (sq(p) * vs).sum(-1, keepdim=True)) + sq(1e-6 * p) + sq(_ulp(p, fl))
    att = D(A['att'])
    vatt = (vp @ sq(V) + sq(p) @ vV + sq(ACC * (p @ V.abs()))).permute(0, 2, 1, 3).reshape(M, C) + sq(_ulp(att, fl))
    g1r, g2r, s2r = rows(g1[:, :C]), rows(g2[:, :C]), rows(s2[:, :C])
    wpd, w1d, w2d = D(d['wp']), D(d['w1']), D(d['w2'])
    acc = lambda a_, w_: sq(ACC * (a_.abs() @ w_.abs().T))
    x2 = D(A['x2'])
    vx2 = sq(g1r) * (vatt @ sq(wpd).T + acc(att, wpd)) + sq(1e-6 * (x2.abs() + g1r.abs() * (att.abs() @ wpd.abs().T + D(d['bp']).abs())))
    xc = x2 - x2.mean(-1, keepdim=True)
    rstd = (xc.pow(2).mean(-1, keepdim=True) + 1e-6).rsqrt()
    xh = xc * rstd
    vxh = 3 * sq(rstd) * (vx2 + vx2.mean(-1, keepdim=True) / C + sq(xh) * (sq(xh) * vx2).mean(-1, keepdim=True) / C)
    xn2, hid = D(A['xn']), D(A['hid'])
    vxn2 = sq(s2r + 1) * vxh + sq(_ulp(xn2, fl))
    vhid = 1.13 ** 2 * (vxn2 @ sq(w1d).T + acc(xn2, w1d)) + sq(1e-6 * hid) + sq(_ulp(hid, fl))
    xo = D(A['x'])
    vx = 2 * (vx2 + sq(g2r) * (vhid @ sq(w2d).T + acc(hid, w2d))) + sq(1e-6 * (xo.abs() + g2r.abs() * (hid.abs() @ w2d.abs().T + D(d['b2']).abs())))
    _ratio(f'{fl} block x vs twin', (xo - tx).abs(), 8 * vx.sqrt())


# ---------------------------------------------------------------------------------------------------------------------
# (forced tile, persistent kernel on): -1 = automatic choice; 0: 128x128, 1: 64-row / 32x32 kernels, 2: 256x256, 3: 192x256
RUNS = [(-1, 1), (0, 1), (1, 1), (2, 1), (2, 0), (3, 1)]


def _batched_operands(case, B, dt, g):
    """(A, lda, W, ldw, bias, out_f16, M, N, K, batch, sA, sW, sO, ldo): flat operand buffers, every slice with its own data.
    'scores' / 'vt' / 'pv' are the three batched products of the 16-bit attnblock (engine._Ops16) at HW = 256, C = 640, with its exact arguments."""
    HW, C = 256, 640
    r16 = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dt).cuda()
    if case == 'scores':              # q . k^T: both operands inside the [B*HW, 2C] q|k projection, fp32 out
        qk = r16(B * HW * 2 * C)
        return qk, 2 * C, qk[C:], 2 * C, None, 0, HW, HW, C, B, HW * 2 * C, HW * 2 * C, HW * HW, HW
    if case == 'vt':                  # V^T = Wv . xn^T per image: the weight shared (sA = 0), 16-bit out, no bias
        w = r16(3 * C * C, sc=C ** -0.5)
        return w[2 * C * C:], C, r16(B * HW * C), C, None, 1, C, HW, C, B, 0, HW * C, C * HW, HW
    if case == 'pv':                  # p . V with v's bias as a column bias, 16-bit out
        p = torch.softmax(torch.randn(B, HW, HW, generator=g) * 2, dim=-1).to(dt).cuda().view(-1)
        return p, HW, r16(B * C * HW), HW, (torch.randn(C, generator=g) * 0.05).cuda(), 1, HW, C, HW, B, HW * HW, C * HW, HW * C, C
    if case == 'ragged':              # partial tiles, lda > K, ldo > N, gaps between the output slices (sO > M * ldo)
        M, N, K, lda, ldo = 200, 132, 128, 136, 140
        sA, sW, sO = M * lda + 8, N * K + 8, M * ldo + 20
        A = torch.full((B * sA,), 8.0, dtype=dt, device='cuda')                    # the gaps hold 8.0: reading them shows in the sums
        A.as_strided((B, M, K), (sA, lda, 1)).copy_(r16(B, M, K))
        return A, lda, r16(B * sW), K, (torch.randn(N, generator=g) * 0.2).cuda(), 1, M, N, K, B, sA, sW, sO, ldo
    if case == 'ragged_tight':        # the same partial tiles with nothing behind the last slice: A, W and the output end with their last batch's last element
        M, N, K, lda, ldo = 200, 132, 128, 136, 140
        sA, sW, sO = M * lda + 8, N * K + 8, M * ldo + 20
        A = torch.full(((B - 1) * sA + (M - 1) * lda + K,), 8.0, dtype=dt, device='cuda')
        A.as_strided((B, M, K), (sA, lda, 1)).copy_(r16(B, M, K))
        return A, lda, r16((B - 1) * sW + N * K), K, (torch.randn(N, generator=g) * 0.2).cuda(), 1, M, N, K, B, sA, sW, sO, ldo
    assert case == 'whole256'         # whole 256x256 tiles: forced tile 2 runs the persistent kernel with blockIdx.z > 0
    return r16(B * 512 * 128), 128, r16(B * 512 * 128, sc=0.1), 128, None, 0, 512, 512, 128, B, 512 * 128, 512 * 128, 512 * 512, 512


@pytest.mark.parametrize('fl', ['f16', 'bf16'])
@pytest.mark.parametrize('case,B', [('scores', 2), ('vt', 2), ('pv', 2), ('scores', 64), ('vt', 64), ('pv', 64), ('ragged', 3), ('whole256', 4), ('ragged_tight', 3)])
def test_gemm16_batched(fl, case, B):
    """varhip_gemm_nt_{f16,bf16} with batch > 1 on every tile (forced 0-3, automatic, 256x256 with and without the persistent kernel):
    all runs the same bits, every slice against float64 within test_gemm16_against_float64's bar (ACC * sum |a||w| + 1e-6, + U |ref| for a
    16-bit result), the gaps of a strided output untouched, and each run in the kernel family its tile implies (timing table: 'gemm16' is the
    persistent kernel alone)"""
    hip = _hip()
    so = hip.lib().so
    dt, U = FLAV[fl]
    g = torch.Generator().manual_seed(B * 31 + len(case))
    A, lda, W, ldw, bias, o16, M, N, K, batch, sA, sW, sO, ldo = _batched_operands(case, B, dt, g)
    sentinel = -7.0
    first = None
    for tile, persist in RUNS:
        out = torch.full(((batch - 1) * sO + (M - 1) * ldo + N if case == 'ragged_tight' else batch * sO,), sentinel, dtype=dt if o16 else torch.float32, device='cuda')
        so.varhip_gemm16_force_tile(tile); so.varhip_gemm16_persistent(persist)
        hip.timing_reset(); hip.timing_enable(True)
        try:
            util.guarded_call('gemm_nt_' + fl, A, lda, W, ldw, bias, out, ldo, o16, M, N, K, 0, None, 0, 0, None, 0, 1, batch, sA, sW, sO)
        finally:
            hip.timing_enable(False); so.varhip_gemm16_force_tile(-1); so.varhip_gemm16_persistent(1)
        t = hip.timing_read()
        # (the automatic choice never lands on the persistent kernel here: rows or N are not whole 256 tiles, or a smaller tile wins)
        fam = 'gemm16' if (tile == 2 and persist and M % 256 == 0 and N % 256 == 0) else 'gemm16_small'
        other = 'gemm16_small' if fam == 'gemm16' else 'gemm16'
        assert t[fam]['launches'] == 1 and t[other]['launches'] == 0, f'tile {tile} persist {persist}: expected one {fam} launch, {t}'
        if first is None:
            first = out
            continue
        assert torch.equal(out, first), f'tile {tile} persistent {persist}: {int((out != first).sum())} elements differ from the automatic choice'
    As = A.as_strided((batch, M, K), (sA, lda, 1)).double()
    Ws = W.as_strided((batch, N, K), (sW, ldw, 1)).double()
    ref = As @ Ws.transpose(1, 2) + (bias.double() if bias is not None else 0.0)
    bar = ACC * (As.abs() @ Ws.abs().transpose(1, 2)) + 1e-6 + (U * ref.abs() if o16 else 0.0)
    got = first.as_strided((batch, M, N), (sO, ldo, 1)).double()
    _ratio(f'{fl} {case} B={B}', (got - ref).abs(), bar)
    written = torch.zeros(first.numel(), dtype=torch.bool, device='cuda')
    written.as_strided((batch, M, N), (sO, ldo, 1)).fill_(True)
    assert bool((first[~written] == sentinel).all()), 'an element outside the output slices was written'


def test_gemm16_batched_rejects_resid_and_gamma():
    hip = _hip()
    from var_amd.hip import VarHipError
    a = torch.zeros(2, 64, 64, dtype=torch.float16, device='cuda'); o = torch.zeros(2, 64, 64, device='cuda'); gm = torch.ones(1, 64, device='cuda')
    for fl, dt in (('f16', torch.float16), ('bf16', torch.bfloat16)):
        a = a.to(dt)
        with pytest.raises(VarHipError):
            hip.call('gemm_nt_' + fl, a, 64, a, 64, None, o, 64, 0, 64, 64, 64, EPI_RESID, o, 64, 0, None, 0, 1, 2, 4096, 4096, 4096)
        with pytest.raises(VarHipError):
            hip.call('gemm_nt_' + fl, a, 64, a, 64, None, o, 64, 0, 64, 64, 64, 0, None, 0, 0, gm, 64, 1, 2, 4096, 4096, 4096)


# ---------------------------------------------------------------------------------------------------------------------
def _attnblock_ref(x, wqkv, bqkv, wp, bp, gam, bet, dt, U):
    """AttnBlock.forward (basic_vae.py:73-85) in float64 on channels-last x [B, H, W, C], and the bar of the 16-bit attnblock against it (see
    test_attnblock16_against_float64) -> (ref [B, HW, C], bar)"""
    wqkv, wp, bqkv, bp, gam, bet = (t.double() for t in (wqkv, wp, bqkv, bp, gam, bet))
    B, Hh, Ww, C = x.shape
    HW = Hh * Ww
    xd = x.double().view(B, HW, C)
    xg = xd.view(B, HW, 32, C // 32)
    mean = xg.mean(dim=(1, 3), keepdim=True); rstd = (xg.var(dim=(1, 3), unbiased=False, keepdim=True) + 1e-6).rsqrt()
    sc = (rstd * gam.view(32, C // 32)); sh = bet.view(32, C // 32) - mean * sc
    xn = (xg * sc + sh).view(B, HW, C)
    qkv = xn @ wqkv.T + bqkv
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    w = C ** -0.5
    s = q @ k.transpose(1, 2) * w
    p = torch.softmax(s, dim=-1)
    o = p @ v
    ref = xd + o @ wp.T + bp

    var_r = lambda v_: (U * v_.abs()) ** 2 / 3                                         # one 16-bit rounding
    acc = lambda a_, w_: (ACC * (a_.abs() @ w_.abs().T)) ** 2                          # one fp32 accumulation
    vxn = var_r(xn) + (1e-6 * ((xg * sc).abs() + sh.abs()).view(B, HW, C)) ** 2       # + fp32 statistics and apply
    vqk = vxn @ (wqkv[:2 * C] ** 2).T + acc(xn, wqkv[:2 * C]) + var_r(qkv[..., :2 * C])
    vt = v - bqkv[2 * C:]                                                              # V^T is rounded without its bias
    vv = vxn @ (wqkv[2 * C:] ** 2).T + acc(xn, wqkv[2 * C:]) + var_r(vt)
    vq, vk = vqk[..., :C], vqk[..., C:]
    vs = (vq @ (k ** 2).transpose(1, 2) + (q ** 2) @ vk.transpose(1, 2) + (ACC * (q.abs() @ k.abs().transpose(1, 2))) ** 2) * w * w + (1e-6 * s) ** 2
    vp = 2 * p ** 2 * (vs + (p ** 2 * vs).sum(-1, keepdim=True)) + (1e-6 * p) ** 2 + var_r(p)
    bias_in_v = bqkv[2 * C:].abs() * (p.to(dt).double().sum(-1, keepdim=True) - 1).abs()
    vo = vp @ (vt ** 2) + (p ** 2) @ vv + (ACC * (p @ vt.abs())) ** 2 + var_r(o) + bias_in_v ** 2
    vy = vo @ (wp ** 2).T + acc(o, wp) + var_r(ref) + (1e-6 * ref) ** 2
    return ref, 8 * vy.sqrt()


@pytest.mark.parametrize('fl', ['f16', 'bf16'])
@pytest.mark.parametrize('pre', ['decoder.mid.attn_1', 'decoder.up.4.attn.1'])
def test_attnblock16_against_float64(fl, pre):
    """DecoderEngine.ops16(flavour).attnblock on the d16 VAE's weights at its 16 x 16 x 640 attention, on a fresh 16-bit input (GroupNorm statistics from a
    statistics pass), against a float64 restatement of AttnBlock.forward (basic_vae.py:73-85) with the same 16-bit weights and fp32 biases / affine.

    Rounding points of the 16-bit attnblock: the GroupNorm output, the q|k projection, V^T, the probabilities, p.V and the output are 16-bit; scores and
    softmax are fp32.  A worst-case chain through the softmax says nothing here: the scores are unnormalised (sum |q||k| / sqrt(C) ~ 16), and
    ACC and U summed in the worst case over every path reach the size of the signal.  The bar is therefore a root-sum-square one: every 16-bit
    rounding is an independent error of variance (U |v|)^2 / 3, every product's accumulation one of standard deviation ACC sum |a||w| (the
    bound the GEMM tests use outright), fp32 element-wise steps 1e-6 |v|; variances are carried in float64 through each product (sum w^2 var)
    and through the softmax as var(d_p) <= 2 p^2 (var(d_s) + sum p^2 var(d_s)).  Bar = 8 sigma.
    v's bias is added to p.V rather than to V (engine.py: V^T's bias would be per row): with sum p = 1 that is exact in the reference's
    arithmetic; against a bias-in-V form with rounded p it differs by |b_v| |sum p16 - 1| <= 0.05 * 1e-3, which the bar also carries.

    Then the same call at B = 64 whose first two images are the B = 2 input: the same bits (GroupNorm's statistics are reduced per image in a
    fixed chunk order, softmax per row, and every GEMM tile gives the same bits: test_gemm16_batched)."""
    z, meta = util.load_case('d16_full')
    vae, var = _models(meta)
    eng = vae._decoder_engine()
    eng.refresh(); ops = eng.ops16(fl)
    dt, U = FLAV[fl]
    B, Hh, C = 2, 16, 640
    HW = Hh * Hh
    g = torch.Generator().manual_seed(7 + len(pre))
    x64 = (torch.randn(64, Hh, Hh, C, generator=g) * 1.5 + 0.4).to(dt).cuda()
    x = x64[:B].contiguous()
    with torch.inference_mode():
        eng._gn_part = None
        y = ops.attnblock(x, pre, B, Hh, Hh).clone()
        eng._gn_part = None
        y64 = ops.attnblock(x64, pre, 64, Hh, Hh)
    assert torch.equal(y64[:B], y), f'B = 64 vs B = 2: {int((y64[:B] != y).sum())} elements differ'

    D = lambda t: t.double()
    ref, bar = _attnblock_ref(x, ops.w16[pre + '.qkv.weight'], eng.w[pre + '.qkv.bias'], ops.w16[pre + '.proj_out.weight'],
                              eng.w[pre + '.proj_out.bias'], eng.w[pre + '.norm.weight'], eng.w[pre + '.norm.bias'], dt, U)
    _ratio(f'{fl} attnblock16 {pre}', (D(y).view(B, HW, C) - ref).abs(), bar)
