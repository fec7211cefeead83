"""Plain float64 references of the training-side NHWC kernels (csrc/train_ops.hip, and the max-pool / bilinear forward of
csrc/elementwise.hip), written from each operation's definition, plus Python mirrors of the launch geometry so that a test case can
assert which branch of a kernel it reaches.  Pinned to torch's fp64 autograd and to ATen's max-pool rules by tests/test_train_ops_cpu.py;
used on the GPU by tests/test_gpu_train_ops.py.  Tensors are [M][C] (or [B][H][W][C]) with C innermost, as the kernels see them."""
import numpy as np
import torch

ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
F64 = torch.float64


def rel_err(got, ref):
    """max|got - ref| / max|ref| -- the figure of test_bn_pool_upsample_backward_at_full_size."""
    ref = torch.as_tensor(ref).double()
    got = torch.as_tensor(got).to(ref.device).double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------
def bn_fwd(y, gamma, beta, eps, momentum=0.1, run_mean=None, run_var=None, residual=None, relu=False):
    """Batch-statistics BatchNorm over the rows of y [M][C].  Returns a dict: sums [2][C] (sum x, sum x^2), mean, var (biased, clamped
    at 0), invstd, run_mean / run_var (None without running statistics; the unbiased variance, M = 1 keeps the biased one), out."""
    y = y.to(F64)
    m = y.shape[0]
    s, ss = y.sum(0), (y * y).sum(0)
    mean = s / m
    var = (ss / m - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))          # (eps reaches the kernel as a float32)
    res = dict(sums=torch.stack([s, ss]), mean=mean, var=var, invstd=invstd, run_mean=None, run_var=None)
    if run_mean is not None:
        unbiased = var * m / (m - 1) if m > 1 else var
        res['run_mean'] = (1.0 - momentum) * run_mean.to(F64) + momentum * mean
        res['run_var'] = (1.0 - momentum) * run_var.to(F64) + momentum * unbiased
    out = (y - mean) * invstd * gamma.to(F64) + beta.to(F64)
    if residual is not None:
        out = out + residual.to(F64)
    if relu:
        out = out.clamp_min(0.0)
    res['out'] = out
    return res


def bn_bwd(dout, y, mean, invstd, gamma, mask=None):
    """mask: bool [M][C] (`out > 0` of the tensor the kernel is given) or None.  Returns dy, dres, dgamma, dbeta in float64."""
    dz = dout.to(F64)
    if mask is not None:
        dz = torch.where(mask, dz, torch.zeros_like(dz))
    m = y.shape[0]
    xhat = (y.to(F64) - mean.to(F64)) * invstd.to(F64)
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dy = gamma.to(F64) * invstd.to(F64) * (dz - dbeta / m - xhat * dgamma / m)
    return dy, dz, dgamma, dbeta


def bn_bwd_sum_operands(dout, y, mean, invstd, mask=None):
    """The two fp64 column sums of the backward statistics pass over the operands the kernel documents: dz exactly (dout or 0) and
    xhat = (y - mean) * invstd formed in float32, then widened.  [2][C]: sum dz, sum dz * xhat."""
    dz = dout if mask is None else torch.where(mask, dout, torch.zeros_like(dout))
    xhat = (y - mean) * invstd
    assert xhat.dtype == torch.float32
    return torch.stack([dz.to(F64).sum(0), (dz.to(F64) * xhat.to(F64)).sum(0)])


def act_bias_bwd(dy, y, act):
    """dz = dy * act'(y) (y is the activation's OUTPUT), dbias = column sums of dz."""
    dz = dy.to(F64)
    if act == ACT_RELU:
        dz = torch.where(y > 0, dz, torch.zeros_like(dz))
    elif act == ACT_TANH:
        dz = dz * (1.0 - y.to(F64) ** 2)
    return dz, dz.sum(0)


# ---- MaxPool2d(3, 2, 1) ---------------------------------------------------------------------------------------------------------
def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def maxpool_fwd(x):
    """x [B][H][W][C] (numpy or torch) -> (out [B][Ho][Wo][C], arg uint8 [B][Ho][Wo][C]).  arg = 3*dy + dx in window coordinates under
    ATen's rule: the running maximum starts at -inf ON the first valid element, a later value wins if it is larger or NaN."""
    x = np.asarray(x, dtype=np.float64)
    b, h, w, c = x.shape
    ho, wo = pool_out(h), pool_out(w)
    out = np.empty((b, ho, wo, c), np.float64)
    arg = np.empty((b, ho, wo, c), np.uint8)
    for oh in range(ho):
        for ow in range(wo):
            best, pos = None, None
            for dy in range(3):
                for dx in range(3):
                    ih, iw = 2 * oh - 1 + dy, 2 * ow - 1 + dx
                    if not (0 <= ih < h and 0 <= iw < w):
                        continue
                    v = x[:, ih, iw, :]
                    if best is None:
                        best, pos = np.full_like(v, -np.inf), np.full(v.shape, 3 * dy + dx, np.uint8)
                    with np.errstate(invalid='ignore'):
                        take = (v > best) | np.isnan(v)
                    best = np.where(take, v, best)
                    pos = np.where(take, np.uint8(3 * dy + dx), pos)
            out[:, oh, ow, :], arg[:, oh, ow, :] = best, pos
    return out, arg


def maxpool_bwd(arg, dy, h, w):
    """Every window's gradient goes to the input pixel its arg byte names.  float64 [B][H][W][C]."""
    arg, dy = np.asarray(arg), np.asarray(dy, dtype=np.float64)
    b, ho, wo, c = arg.shape
    dx = np.zeros((b, h, w, c), np.float64)
    bi, ci = np.meshgrid(np.arange(b), np.arange(c), indexing='ij')
    for oh in range(ho):
        for ow in range(wo):
            a = arg[:, oh, ow, :].astype(np.int64)
            ih, iw = 2 * oh - 1 + a // 3, 2 * ow - 1 + a % 3
            assert (ih >= 0).all() and (ih < h).all() and (iw >= 0).all() and (iw < w).all(), 'an arg byte names a padding position'
            np.add.at(dx, (bi, ih, iw, ci), dy[:, oh, ow, :])
    return dx


def maxpool_flat_index(arg, w):
    """ATen's index (ih * W + iw of the input plane) of every arg byte."""
    arg = np.asarray(arg).astype(np.int64)
    _, ho, wo, _ = arg.shape
    oh, ow = np.arange(ho)[None, :, None, None], np.arange(wo)[None, None, :, None]
    return (2 * oh - 1 + arg // 3) * w + (2 * ow - 1 + arg % 3)


# ---- bilinear x2 ----------------------------------------------------------------------------------------------------------------
def bilinear_matrix(n_in, align_corners):
    """[2 * n_in][n_in] float64 interpolation matrix of one axis, ATen's area_pixel_compute_source_index."""
    n_out = 2 * n_in
    mat = np.zeros((n_out, n_in), np.float64)
    for d in range(n_out):
        if align_corners:
            src = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        else:
            src = max(0.0, (d + 0.5) * n_in / n_out - 0.5)
        i0 = min(int(np.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = src - i0
        mat[d, i0] += 1.0 - l1
        mat[d, i1] += l1
    return mat


def bilinear2x_fwd(x, align_corners):
    x = np.asarray(x, dtype=np.float64)
    return np.einsum('ph,qw,bhwc->bpqc', bilinear_matrix(x.shape[1], align_corners), bilinear_matrix(x.shape[2], align_corners), x)


def bilinear2x_bwd(dy, align_corners):
    dy = np.asarray(dy, dtype=np.float64)
    return np.einsum('ph,qw,bpqc->bhwc', bilinear_matrix(dy.shape[1] // 2, align_corners),
                     bilinear_matrix(dy.shape[2] // 2, align_corners), dy)


# ---- head gradient gather -------------------------------------------------------------------------------------------------------
def head_levels(batch, level_pixels, na):
    """Row and anchor offsets of the levels: level l owns batch * level_pixels[l] rows ([b][pixel]) and level_pixels[l] * na anchors."""
    row, anchor = [0], [0]
    for p in level_pixels:
        row.append(row[-1] + batch * p)
        anchor.append(anchor[-1] + p * na)
    return row, anchor


def head_grad_gather(dclass, dbox, dcoef, coef, batch, level_pixels, nc, cd, na, pitch, g_scale=None):
    """dclass [B][N][nc], dbox [B][N][4], dcoef / coef [B][N][cd] (N = na * sum(level_pixels)) -> dz [rows][pitch]: per level the rows
    [b][pixel], per row the columns [na x nc class | na x 4 box | na x cd coefficient (times tanh' = 1 - coef^2) | padding = 0].  Keeps the
    inputs' dtype: in float32 every element is one multiply (class, box) or (dcoef * g) * (1 - t * t), each operation rounded."""
    row, anchor = head_levels(batch, level_pixels, na)
    gc, gb, gm = (g_scale[0], g_scale[1], g_scale[2]) if g_scale is not None else (1.0, 1.0, 1.0)
    dz = torch.zeros(row[-1], pitch, dtype=dclass.dtype)
    for l, p in enumerate(level_pixels):
        a0, a1 = anchor[l], anchor[l + 1]
        blk = dz[row[l]:row[l + 1]].view(batch, p, pitch)
        blk[:, :, :na * nc] = (dclass[:, a0:a1] * gc).reshape(batch, p, na * nc)
        blk[:, :, na * nc:na * (nc + 4)] = (dbox[:, a0:a1] * gb).reshape(batch, p, na * 4)
        t = coef[:, a0:a1]
        blk[:, :, na * (nc + 4):na * (nc + 4 + cd)] = ((dcoef[:, a0:a1] * gm) * (1.0 - t * t)).reshape(batch, p, na * cd)
    return dz


# ---- scatter3, SGD, dgrad weight image ----------------------------------------------------------------------------------------
def scatter3(src, dsts, accumulate):
    """src [n0 + n1 + n2] is cut into the three destinations (copied, or added)."""
    out, at = [], 0
    for d in dsts:
        piece = src[at:at + d.numel()]
        out.append(d + piece if accumulate else piece.clone())
        at += d.numel()
    return out


def sgd_step(p, g, buf, lr, momentum, wd, first):
    """g' = g + wd * p; buf = first ? g' : momentum * buf + g'; p - lr * buf.  float64; lr, momentum, wd as the float32 the kernel gets."""
    lr, momentum, wd = (float(np.float32(v)) for v in (lr, momentum, wd))
    p, g, buf = p.to(F64), g.to(F64), buf.to(F64)
    gg = g + wd * p
    buf = gg if first else momentum * buf + gg
    return p - lr * buf, buf


def dgrad_weight_image(w, cout_pad):
    """OIHW -> [Cin][KH][KW][cout_pad], zero padded (numpy)."""
    w = np.asarray(w)
    cout, cin, kh, kw = w.shape
    out = np.zeros((cin, kh, kw, cout_pad), w.dtype)
    out[..., :cout] = w.transpose(1, 2, 3, 0)
    return out


# ---- launch geometry ------------------------------------------------------------------------------------------------------------
def lane_map(c):
    """Thread (cq, rl) map of k_col_reduce: dict(CQ, RL, idle threads per workgroup, channel passes, threads idle in the last pass)."""
    c4 = c // 4
    cq = min(c4, 256)
    rl = 256 // cq
    passes = -(-c4 // cq)
    return dict(C4=c4, CQ=cq, RL=rl, idle=256 - cq * rl, passes=passes, last_pass_empty=passes * cq - c4)


def col_grid(m, c, rows_per_lane, cap):
    g = -(-m // (lane_map(c)['RL'] * rows_per_lane))
    return max(1, min(g, cap))


def stats_grid(m, c, partials):
    """Grid of k_col_reduce<0|1> (ym_bn_train_fwd / ym_bn_train_bwd): 16 rows per row lane, at most 512 (atomics) / 1024 (partials)."""
    return col_grid(m, c, 16, 1024 if partials else 512)


def bias_grid(m, c, partials):
    """Grid of k_col_reduce<2> (ym_act_bias_bwd): 32 rows per row lane, at most 2048 (atomics) / 1024 (partials)."""
    return col_grid(m, c, 32, 1024 if partials else 2048)


def stats_workspace_bytes(m, c):
    return 16 * c + stats_grid(m, c, True) * 16 * c


def bias_workspace_bytes(m, c):
    return 16 * c + bias_grid(m, c, True) * 16 * c


def col_loops(m, c, grid, unroll):
    """Per row lane of the whole grid, how the row loop of k_col_reduce splits: dict(main = most unrolled iterations of a lane,
    remainder = most remainder iterations, strides = a lane walks more than one row, idle_lanes = lanes without a row)."""
    rl = lane_map(c)['RL']
    stride = grid * rl
    main = rem = idle = 0
    strides = False
    for lane in range(stride):
        n = -(-(m - lane) // stride) if lane < m else 0
        main, rem = max(main, n // unroll), max(rem, n % unroll)
        strides |= n > 1
        idle += n == 0
    return dict(main=main, remainder=rem, strides=strides, idle_lanes=idle)


def col_finish_loops(rows):
    """k_col_finish: slice s (0..15) adds the partial rows s, s + 16, ...; four at a time while k + 48 < rows.  (main, remainder)
    iteration counts of the busiest slice, and whether a slice has no row at all."""
    main = rem = 0
    empty = False
    for s in range(16):
        k = s
        a = b = 0
        while k + 48 < rows:
            a, k = a + 1, k + 64
        while k < rows:
            b, k = b + 1, k + 16
        main, rem, empty = max(main, a), max(rem, b), empty or (a + b == 0)
    return dict(main=main, remainder=rem, empty_slice=empty)


def bn_apply_grid(total, per_thread=4):
    g = -(-total // (256 * per_thread))
    g = max(2, min(g, 8192))
    return (g + 1) & ~1


def quad_loops(total, stride, unroll=4, unrolled=True):
    """Grid-stride walk over `total` quads: the set of (main, remainder) iteration pairs its threads take."""
    kinds = set()
    lo, extra = divmod(total, stride)
    for n in ({lo + 1} if extra else set()) | ({lo} if extra < stride else set()):
        kinds.add((n // unroll, n % unroll) if unrolled else (0, n))
    return kinds


def bwd_apply_geometry(m, c):
    """k_bn_bwd_apply: dict(grid, capped, fixed_c, loops = {(4-quad iterations, remainder iterations)} over the threads)."""
    c4 = c // 4
    total = m * c4
    grid = bn_apply_grid(total)
    stride = grid * 256
    fixed = stride % c4 == 0
    return dict(grid=grid, capped=-(-total // 1024) > 8192, fixed_c=fixed, loops=quad_loops(total, stride, 4, fixed))


def fwd_stats_geometry(m, c):
    """ym_bn_train_fwd_stats: dict(fused = one k_bn_finalize_apply launch, step, grid0 = the grid before it is rounded to a multiple of
    step, grid, loops as in bwd_apply_geometry).  256 * step is a multiple of C/4, so the rounded grid always covers C/4 threads."""
    c4 = c // 4
    total = m * c4
    grid0 = min(-(-total // 2048), 2048)
    step = 1
    while (256 * step) % c4 != 0 and step <= 64:
        step += 1
    if (256 * step) % c4 != 0:
        return dict(fused=False, step=None, grid0=grid0, grid=None, loops=None)
    grid = -(-grid0 // step) * step
    while grid * 256 < c4:
        grid += step
    return dict(fused=True, step=step, grid0=grid0, grid=grid, loops=quad_loops(total, grid * 256))


# ---- case tables (shared by the CPU pins and the GPU tests) ---------------------------------------------------------------------
LANE_SHAPES = [(1, 4), (255, 4), (5000, 4), (37, 24), (338, 96), (77, 352), (50, 1024), (19, 1536), (33, 2048)]
UNROLL_SHAPES = [(16, 1024), (17, 1024), (35, 1024), (50, 1024)]
CAP_SHAPES = [(8292, 1024), (16421, 1024), (32773, 1024), (65539, 1024)]
FWD_STATS_SHAPES = [(37, 64), (338, 96), (40, 28), (77, 352), (9, 268), (1, 2048), (250, 64)]
BWD_APPLY_SHAPES = [(250, 64), (80, 96), (61, 24)]
FINISH_ROWS = [1, 15, 16, 17, 48, 49, 64, 65, 113, 1024]
FINISH_C = [4, 20, 64]
POOL_SHAPES = [(1, 1, 1, 4), (1, 1, 5, 4), (1, 2, 2, 8), (1, 3, 3, 4), (1, 7, 8, 12), (2, 6, 5, 12)]
BILINEAR_SHAPES = [(1, 1, 1, 4), (1, 1, 6, 4), (1, 5, 1, 8), (2, 2, 3, 12), (1, 9, 7, 8)]
SGD_SIZES = [1, 255, 257, 8192 * 256 + 3]
DGRAD_SHAPES = [(35, 5, 3, 64), (32, 1, 1, 32), (81, 7, 3, 96)]
OTHER_MC = [(501, 8), (1, 24), (37, 24), (77, 352), (229377, 256)]      # conditioning, one row, act_bias, the case past the apply cap
ALL_MC = sorted(set(LANE_SHAPES + UNROLL_SHAPES + CAP_SHAPES + FWD_STATS_SHAPES + BWD_APPLY_SHAPES + OTHER_MC))


def bwd_apply_large_m(c=256):
    """Smallest M past the 8192-block cap of k_bn_bwd_apply at which some threads run the 4-quad loop twice and others the remainder."""
    m = 8192 * 1024 // (c // 4)
    while True:
        m += 1
        g = bwd_apply_geometry(m, c)
        if g['capped'] and g['fixed_c'] and any(a >= 2 for a, _ in g['loops']) and any(b > 0 for _, b in g['loops']):
            return m


def bn_inputs(m, c, seed, device='cpu'):
    """y, gamma, beta, residual, dout, and a post-ReLU `out` whose mask takes both values in every channel (rows 0 and 1; with one row
    the channels alternate)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(m, c, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    res, dout = torch.randn(m, c, generator=g), torch.randn(m, c, generator=g)
    out = torch.relu(torch.randn(m, c, generator=g))
    if m > 1:
        out[0], out[1] = 1.0, 0.0
    else:
        out[0] = (torch.arange(c) % 2).float()
    return tuple(t.to(device) for t in (y, gamma, beta, res, dout, out))


def big_bn_inputs(m, c, seed, device):
    """The same roles drawn on `device` (the cap cases: too large to ship from the host in a quick test)."""
    g = torch.Generator(device=device).manual_seed(seed)
    y = torch.randn(m, c, generator=g, device=device) * 2 + 0.5
    gamma, beta = torch.rand(c, generator=g, device=device) + 0.5, torch.randn(c, generator=g, device=device) * 0.1
    dout = torch.randn(m, c, generator=g, device=device)
    out = torch.relu(torch.randn(m, c, generator=g, device=device))
    out[0], out[1] = 1.0, 0.0
    return y, gamma, beta, dout, out


def mask_takes_both_values(out):
    pos = (out > 0)
    if out.shape[0] > 1:
        return bool(pos.any(0).all()) and bool((~pos).any(0).all())
    return bool(pos.any()) and bool((~pos).any())


def conditioning_input(m, c, seed):
    """y [m][c] whose channel 0 is the constant 1.5 and whose channel 1 has mean 100 and std 0.1.  Channel 1 is made of pairs 100 +- d (d a
    multiple of 2^-16, one row of exactly 100 when m is odd), so its mean is exactly 100 in every precision: the case is about the variance
    (E[x^2] - E[x]^2 loses six of fp64's sixteen digits there), and a mean that float32 cannot hold would put up to ulp(100)/2 * invstd =
    4e-5 into `out` through save_mean's own rounding, which no kernel that publishes a float32 mean can avoid."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(m, c, generator=g)
    y[:, 0] = 1.5
    d = torch.round(torch.randn(m // 2, generator=g) * 0.1 * 65536) / 65536
    col = torch.cat([100.0 + d, 100.0 - d] + ([torch.tensor([100.0])] if m % 2 else []))
    y[:, 1] = col[torch.randperm(m, generator=g)]
    return y


def pool_input(shape, seed):
    """Post-ReLU values on a grid of halves: most windows hold ties, many hold several zeros.  (1,3,3,4) is all equal."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.round(torch.randn(shape, generator=g) * 2) / 2)
    if tuple(shape) == (1, 3, 3, 4):
        x = torch.full(shape, 0.75)
    return x


def pool_grad(x, seed):
    """Gradient of the pooled tensor on a grid of quarters: sums of up to four of them are exact in float32."""
    b, h, w, c = x.shape
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (b, pool_out(h), pool_out(w), c), generator=g).float() / 4


def window(x, oh, ow):
    """The valid elements of window (oh, ow) of x [B][H][W][C], in scan order: [B][n][C]."""
    _, h, w, _ = x.shape
    cells = [(2 * oh - 1 + dy, 2 * ow - 1 + dx) for dy in range(3) for dx in range(3)]
    return torch.stack([x[:, i, j, :] for i, j in cells if 0 <= i < h and 0 <= j < w], 1)


def windows_with_ties(x):
    """How many (window, batch, channel) triples hold their maximum more than once."""
    _, h, w, _ = x.shape
    n = 0
    for oh in range(pool_out(h)):
        for ow in range(pool_out(w)):
            v = window(x, oh, ow)
            n += int(((v == v.max(1, keepdim=True).values).sum(1) > 1).sum())
    return n


def pool_inf_input(seed=3):
    """(1,6,6,4): the border window (0,0) (valid elements rows 0-1 x columns 0-1; position 0 is padding) and the interior window (2,2)
    (rows 3-5 x columns 3-5) hold nothing but -inf."""
    x = pool_input((1, 6, 6, 4), seed) + 0.25
    x[:, 0:2, 0:2] = float('-inf')
    x[:, 3:6, 3:6] = float('-inf')
    return x


def pool_nan_input(seed=4):
    """(1,6,6,4): window (0,0) holds one NaN (at (1,0)); window (2,2) holds two (at (3,4) and (5,3)); window (0,2) holds three in one row
    (at (1,3), (1,4), (1,5))."""
    x = pool_input((1, 6, 6, 4), seed)
    for i, j in ((1, 0), (3, 4), (5, 3), (1, 3), (1, 4), (1, 5)):
        x[:, i, j] = float('nan')
    return x
