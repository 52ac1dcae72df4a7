"""What tests/test_patch_cpu.py and tests/test_patch_kernels_gpu.py share: a numpy restatement of varhip_act_patch_f32's directive semantics
(include/var_hip.h), the mean's summation order included, and the deck of cases both sides run."""
import numpy as np

ZERO, MEAN = -1, -2


def apply(act, rows, l, width, dirs):
    """act (rows * l, ld) fp32 -> a copy with the directives dirs (n, 4) int32 (row, c0, c1, src) applied, one after the other.
    zero: +0.0; mean: s = act[0], s = s + act[t] for t = 1 .. l - 1 in float32 (numpy rounds every add), m = s / float32(l); src >= 0: the
    source row's tokens.  A directive that names anything outside the matrix, or a bound that is no multiple of 4, writes nothing."""
    out = np.array(act, dtype=np.float32, copy=True)
    for row, c0, c1, src in np.asarray(dirs, dtype=np.int64).reshape(-1, 4):
        if not (0 <= row < rows and -2 <= src < rows and 0 <= c0 < c1 <= width and c0 % 4 == 0 and c1 % 4 == 0):
            continue
        blk = out[row * l:(row + 1) * l, c0:c1]
        if src == ZERO:
            blk[:] = np.float32(0.0)
        elif src == MEAN:
            s = blk[0].copy()
            for t in range(1, l):
                s = (s + blk[t]).astype(np.float32)
            blk[:] = (s / np.float32(l)).astype(np.float32)
        else:
            blk[:] = out[src * l:(src + 1) * l, c0:c1]
    return out


def refused(act, ld, rows, l, width, dirs, n_dir):
    """the contract's VARHIP_EINVAL (n_dir == 0 is success without a launch)"""
    if n_dir == 0:
        return False
    return (n_dir < 0 or act is None or dirs is None or rows < 1 or l < 1 or width < 1 or width > 1 << 22 or ld < width or ld % 4 != 0
            or act.ctypes.data % 16 != 0)


def matrix(rows, l, width, ld, seed):
    """(rows * l, ld) fp32: values of mixed magnitude and sign (the mean's sum then rounds at every add), a few denormals, zeros of both signs;
    NaN in the padding columns width .. ld - 1, which nothing may touch"""
    g = np.random.default_rng(seed)
    a = (g.standard_normal((rows * l, ld)) * np.exp(g.uniform(-6, 6, (rows * l, ld)))).astype(np.float32)
    a[g.random(a.shape) < 0.02] = np.float32(1e-41)
    a[g.random(a.shape) < 0.02] = np.float32(-0.0)
    a[g.random(a.shape) < 0.02] = np.float32(0.0)
    a[:, width:] = np.nan
    return a


def deck():
    """[(name, rows, l, width, ld, dirs (n, 4) int32)]: l in {1, 4, 9, 256}; width 128 with 64-column slices at the first and the last head,
    width 512 whole; ld > width; several directives on one row; every skip rule among directives that apply"""
    cases = []
    for l in (1, 4, 9, 256):
        # width 128 (two heads): rows 0 / 1 zero and mean the first head, rows 2 / 3 the last, row 4 copies row 5's last head, row 5 is a source only
        cases.append((f'heads l={l}', 6, l, 128, 128, [(0, 0, 64, ZERO), (1, 0, 64, MEAN), (2, 64, 128, ZERO), (3, 64, 128, MEAN), (4, 64, 128, 5)]))
        # width 512, the whole width, in each mode; row 3 is the source
        cases.append((f'whole l={l}', 4, l, 512, 512, [(0, 0, 512, ZERO), (1, 0, 512, MEAN), (2, 0, 512, 3)]))
        # ld > width: the padding is NaN and stays; ranges that end at width, and one that is neither head-sized nor 64-aligned
        cases.append((f'padded l={l}', 4, l, 128, 160, [(0, 64, 128, MEAN), (1, 0, 128, ZERO), (2, 4, 100, 3), (2, 100, 128, MEAN)]))
        # several directives on one row (disjoint ranges, all three modes), beside every kind of skipped directive
        cases.append((f'mixed l={l}', 3, l, 512, 512,
                      [(0, 0, 64, ZERO), (0, 64, 128, MEAN), (0, 128, 192, 2), (0, 448, 512, MEAN), (1, 256, 260, ZERO),
                       (-1, 0, 64, ZERO), (3, 0, 64, ZERO), (1, 0, 64, 3), (1, 0, 64, -3), (1, -4, 64, ZERO), (1, 448, 516, ZERO), (1, 64, 64, ZERO),
                       (1, 128, 64, MEAN), (1, 2, 64, ZERO), (1, 0, 62, MEAN), (1, 0, 64, 1 << 20)]))
    return [(n, r, l, w, ld, np.asarray(d, dtype=np.int32).reshape(-1, 4)) for n, r, l, w, ld, d in cases]
