"""Winograd F(2x2,3x3) of the decoder (var_amd/csrc/winograd.hip): the filter transform DecoderEngine.refresh makes (var_amd.engine.wino_filter)
against float64, and the transform algebra the kernel executes against a direct convolution, exactly, on small integer data."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from var_amd.engine import DecoderEngine, wino_filter

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def _unlayout(u, co, ci):
    """[16][Cin/16][Cout][16] -> [4][4][Cout][Cin]"""
    return u.reshape(4, 4, ci // 16, co, 16).permute(0, 1, 3, 2, 4).reshape(4, 4, co, ci)


def test_filter_transform_vs_float64():
    g = torch.Generator().manual_seed(0)
    co, ci = 64, 96
    w = torch.randn(co, 3, 3, ci, generator=g)
    u = wino_filter(w)
    assert u.dtype == torch.float32 and tuple(u.shape) == (16, ci // 16, co, 16) and u.is_contiguous()
    want = np.einsum('ik,jl,oklc->ijoc', G, G, w.double().numpy())
    # computed in float64, rounded once: equal to the correctly rounded float64 result
    assert np.array_equal(_unlayout(u, co, ci).numpy(), want.astype(np.float32))


def _conv_direct(x, w):
    """x [H][W][Cin], w [Cout][3][3][Cin], padding 1 -> [H][W][Cout] (float64)"""
    H, W, _ = x.shape
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    out = np.zeros((H, W, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            out += xp[ky:ky + H, kx:kx + W, :] @ w[:, ky, kx, :].T
    return out


def _conv_wino(x, u):
    """the kernel's algebra: per 2x2 tile V = B^T d B per channel, M[xi] = sum_ci U[xi] V[xi] (wave w holds xi row w), output A^T M A"""
    H, W, _ = x.shape
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    out = np.zeros((H, W, u.shape[2]))
    for ty in range(H // 2):
        for tx in range(W // 2):
            d = xp[2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4, :]                  # [4][4][Cin]
            v = np.einsum('ir,rcs,jc->ijs', BT, d, BT)                        # B^T d B
            m = np.einsum('ijos,ijs->ijo', u, v)                              # [4][4][Cout]
            out[2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2, :] = np.einsum('ai,ijo,bj->abo', AT, m, AT)
    return out


@pytest.mark.parametrize('H,W', [(4, 4), (6, 8)])
def test_winograd_identity_exact_on_integers(H, W):
    """small integer inputs and kernels: U then holds multiples of 1/4 and every intermediate is exact in float64, so the Winograd form
    equals the direct convolution bit for bit, padding rows and columns included"""
    rng = np.random.default_rng(0)
    ci, co = 32, 32
    x = rng.integers(-8, 9, size=(H, W, ci)).astype(np.float64)
    w = rng.integers(-4, 5, size=(co, 3, 3, ci)).astype(np.float32)
    u = _unlayout(wino_filter(torch.from_numpy(w)), co, ci).double().numpy()
    assert np.array_equal(u * 4, np.round(u * 4))                             # U = G g G^T holds quarters, exact in fp32 here
    assert np.array_equal(_conv_wino(x, u), _conv_direct(x, w.astype(np.float64)))


def test_shape_rule():
    e = DecoderEngine.__new__(DecoderEngine)
    assert e.wino_ok(16, 16, 640, 640) and e.wino_ok(256, 256, 160, 160) and e.wino_ok(64, 64, 160, 320)
    assert not e.wino_ok(8, 8, 64, 64) and not e.wino_ok(24, 24, 64, 64) and not e.wino_ok(32, 32, 48, 64) and not e.wino_ok(32, 32, 64, 16)


def _decoder_with_shapes(ch=160, P=16):
    """a DecoderEngine whose packed-weight table holds the bench VQVAE's decoder shapes (meta tensors: no data, no GPU); refresh() is a no-op"""
    from types import MethodType
    from var_amd.models.vqvae import VQVAE
    with torch.device('meta'):
        vae = VQVAE(vocab_size=4096, z_channels=32, ch=ch, test_mode=True, share_quant_resi=4, v_patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, P))
    e = DecoderEngine.__new__(DecoderEngine)
    w = {}
    for k, v in vae.state_dict().items():
        if not k.startswith(DecoderEngine.PREFIXES):
            continue
        if v.dim() == 4 and v.shape[-1] == 3:
            w[k] = torch.empty(v.shape[0], 3, 3, (v.shape[1] + 31) // 32 * 32, device='meta')
        elif v.dim() == 4:
            w[k] = torch.empty(v.shape[0], v.shape[1], device='meta')
        else:
            w[k] = v
    e.w = w
    e.nlev = 1 + max(int(k.split('.')[2]) for k in w if k.startswith('decoder.up.'))
    e.refresh = MethodType(lambda self: None, e)
    return e


def _executed_without_winograd(e, P):
    """the count before the Winograd path existed: the reference count with the Upsample2x convs folded to 4 taps"""
    f, hw = e.flops_per_image_reference(P), P * P
    for lev in reversed(range(e.nlev)):
        if lev != 0:
            hw *= 4
            co, _, _, ci = e.w[f'decoder.up.{lev}.upsample.conv.weight'].shape
            f -= 2.0 * hw * co * 5 * ci
    return f


def test_executed_flops_count_winograd_only_in_f32():
    """only an f32 decode runs the Winograd kernel: the 16-bit count is the one without it; the f32 count drops by 5/9 of every ResnetBlock
    conv (all of them tile into 16 x 16 patches at P = 16, ch = 160); the precision defaults to the last one the engine was told about"""
    from types import SimpleNamespace
    from var_amd.engine import SamplingEngine
    P = 16
    e = _decoder_with_shapes(P=P)
    base = _executed_without_winograd(e, P)
    assert e.flops_per_image_executed(P, 'f16') == base and e.flops_per_image_executed(P, 'bf16') == base
    resblock = 0.0
    for k in e.w:
        if k.endswith(('.conv1.weight', '.conv2.weight')):
            co, _, _, ci = e.w[k].shape
            lev = k.split('.')[2] if k.startswith('decoder.up.') else None
            hw = (P * 2 ** (e.nlev - 1 - int(lev))) ** 2 if lev is not None else P * P
            resblock += 2.0 * hw * co * 9 * ci
    wino = e.flops_per_image_executed(P, 'f32')
    assert abs((base - wino) - resblock * 5 / 9) <= 1e-9 * base
    e.winograd = False
    assert e.flops_per_image_executed(P, 'f32') == base
    e.winograd = True
    # default precision: what the owning SamplingEngine was last set to (bench.py sets it before it prices each mode)
    se = SimpleNamespace(policy='f32', precision='f32', dec=e, _ws={}, _ws_tf={})
    SamplingEngine.set_precision(se, 'bf16')
    assert e.flops_per_image_executed(P) == base
    SamplingEngine.set_precision(se, 'f32')
    assert e.flops_per_image_executed(P) == wino
    SamplingEngine.set_precision(se, 'auto')                        # resolved per call: the count keeps the last explicit / decoded precision
    assert e.flops_per_image_executed(P) == wino
