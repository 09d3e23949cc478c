"""UpdateBlock (conv.py:588-616, + the residual adds of cgvae.py:122-123) restated in numpy fp64 from the formulas in the header
of csrc/update.hip, one function per launch, and every output with an A-PRIORI fp32 error bound beside it.

A quantity is a ``Q``: ``val`` (fp64, the exact formula on the inputs given) and ``err`` (a bound on |what the fp32 kernel
stores - val|).  The bound of one launch on exact inputs is

    (rounded fp32 operations on the longest path to the element) x 2^-24 x (sum of the absolute values of the terms)

-- the standard forward bound of a sum of products, each operation count written beside the kernel line it counts.  A fused
multiply-add rounds once where the count has two, so contraction only stays further inside.  Inputs that carry an error
of their own (``Q`` in, the composed ``block``) add its first-order propagation, with magnitudes |x| + err in place of |x|
so that nothing second-order is dropped.  Nothing here was fitted to a GPU run.

Layout: an operand that the kernels read with a row stride is passed as its whole [3 n, ld] buffer plus the column where
its F columns start (ld = F, col = 0: a buffer of its own; ld = 2 F: U at col 0 and Vv at col F of one product)."""
import numpy as np

U32 = 2.0 ** -24              # unit roundoff of fp32, round to nearest
EPS = 1e-10                   # conv.py:600 (v_v ** 2 + 1e-10): fp32 holds it within U32 relative, counted with its add


class Q:
    """value and bound on |fp32 result - value|; + and * propagate input errors only (the caller adds the launch's own
    rounding with ``rounded``)."""

    def __init__(self, val, err=None):
        self.val = np.asarray(val, dtype=np.float64)
        self.err = np.zeros_like(self.val) if err is None else np.broadcast_to(np.asarray(err, dtype=np.float64), self.val.shape).copy()

    @property
    def mag(self):
        return np.abs(self.val) + self.err

    @property
    def shape(self):
        return self.val.shape

    def view(self, fn):
        return Q(fn(self.val), fn(self.err))

    def __getitem__(self, ix):
        return Q(self.val[ix], self.err[ix])

    def __add__(self, o):
        o = q(o)
        return Q(self.val + o.val, self.err + o.err)

    def __mul__(self, o):
        o = q(o)
        return Q(self.val * o.val, np.abs(self.val) * o.err + np.abs(o.val) * self.err + self.err * o.err)

    def sum(self, axis):
        return Q(self.val.sum(axis), self.err.sum(axis))

    def rounded(self, count, mag):
        return Q(self.val, self.err + count * U32 * mag)


def q(x):
    return x if isinstance(x, Q) else Q(x)


def _div(a, b):
    """a / b without its rounding; b must stay away from zero by more than its own error"""
    assert (np.abs(b.val) > b.err).all()
    val = a.val / b.val
    return Q(val, (a.err + np.abs(val) * b.err) / (np.abs(b.val) - b.err))


def _matmul(a, b):
    a, b = q(a), q(b)
    return Q(a.val @ b.val, a.err @ np.abs(b.val) + a.mag @ b.err)


def _zeros(*shape):
    return Q(np.zeros(shape))


def node_rows(buf, n, F, ld, col):
    """[3 n, ld] buffer -> its columns col .. col + F as [n, 3, F] (row = node * 3 + xyz)"""
    buf = q(buf)
    assert buf.val.size == 3 * n * ld and col + F <= ld
    return buf.view(lambda t: t.reshape(n, 3, ld)[:, :, col:col + F])


# ------------------------------------------------------------------------------------------------ the six launches
def rows_from_vec(v, n, F):
    """update_rows_from_vec: v [n, F, 3] -> rows [3 n, F]; a copy, 0 rounded operations"""
    return q(v).view(lambda t: t.reshape(n, F, 3).transpose(0, 2, 1).reshape(3 * n, F))


def vec_from_rows(rows, n, F, res=None):
    """update_vec_from_rows: rows [3 n, F] (+ res [n, F, 3]) -> vec [n, F, 3]"""
    out = q(rows).view(lambda t: t.reshape(n, 3, F).transpose(0, 2, 1))
    if res is None:
        return out                                               # a copy: 0
    r = q(res).view(lambda t: t.reshape(n, F, 3))
    return (out + r).rounded(1, out.mag + r.mag)                 # `x += t.x`: 1 add


def norm_stack_fwd(s, Vv, n, F, ld, col=0):
    """update_norm_stack_fwd: stack = [ s | sqrt(sum_k (Vv_k^2 + 1e-10)) ]  [n, 2 F]"""
    s, vv = q(s).view(lambda t: t.reshape(n, F)), node_rows(Vv, n, F, ld, col)
    nrm = np.sqrt((vv.val ** 2 + EPS).sum(1))
    prop = vv.err.sum(1)            # the norm of (x, y, z, sqrt(3e-10)) is 1-Lipschitz in each component
    # `sqrtf(((x * x + 1e-10f) + (y * y + 1e-10f)) + (z * z + 1e-10f))`: 3 squares, 3 `+ 1e-10f`, 2 adds, 1 sqrt = 9; the
    # terms are all positive, so their sum of absolute values under the root is the norm itself
    nq = Q(nrm, prop).rounded(9, nrm + prop)
    return Q(np.concatenate([s.val, nq.val], 1), np.concatenate([s.err, nq.err], 1))     # `stack[..] = s[idx]`: a copy


def norm_stack_bwd(gstack, Vv, stack, n, F, ld, col=0, g_res=None, gVv_old=None, accumulate=0):
    """update_norm_stack_bwd: g_s [n, F] = gstack[:, :F] (+ g_res); gVv [n, 3, F] (+)= gstack[:, F:] / vnorm * Vv.
    ``gVv_old``: what the gVv columns held ([3 n, ld] buffer, read at ``col``), needed when ``accumulate``."""
    gst, st, vv = q(gstack).view(lambda t: t.reshape(n, 2 * F)), q(stack).view(lambda t: t.reshape(n, 2 * F)), node_rows(Vv, n, F, ld, col)
    g_s = gst[:, :F]                                             # `g_s[idx] = gs`: a copy
    if g_res is not None:
        r = q(g_res).view(lambda t: t.reshape(n, F))
        g_s = (g_s + r).rounded(1, g_s.mag + r.mag)              # `gs += slice_sum_at(g_res, idx)`: 1 add
    t = _div(gst[:, F:], st[:, F:])                              # `t = gstack / stack`: 1 division
    term = t.view(lambda a: a[:, None, :]) * vv                  # `t * vv[0]`: 1 multiply per component
    if not accumulate:
        return g_s, term.rounded(2, term.mag)                    # division + multiply = 2
    old = node_rows(gVv_old, n, F, ld, col)
    return g_s, (old + term).rounded(3, old.mag + term.mag)      # `o[0] += t * vv[0]`: division + multiply + add = 3


def _gate_operands(Ubuf, Vbuf, a, n, F, ld, u_col, v_col):
    u, vv = node_rows(Ubuf, n, F, ld, u_col), node_rows(Vbuf, n, F, ld, v_col)
    a3 = q(a).view(lambda t: t.reshape(n, 3, F))
    return u, vv, a3[:, 0], a3[:, 1], a3[:, 2]


def gate_fwd(Ubuf, Vbuf, a, n, F, ld, u_col=0, v_col=0, s_res=None, v_res=None):
    """update_gate_fwd: dv [n, F, 3] = U a_vv (+ v_res); ds [n, F] = (sum_k U_k Vv_k) a_sv + a_ss (+ s_res)"""
    assert (s_res is None) == (v_res is None)
    u, vv, a_vv, a_sv, a_ss = _gate_operands(Ubuf, Vbuf, a, n, F, ld, u_col, v_col)
    dv = u * a_vv.view(lambda t: t[:, None, :])
    inner = (u * vv).sum(1)
    inner_abs = (u.mag * vv.mag).sum(1)
    ds = inner * a_sv + a_ss
    ds_mag = inner_abs * a_sv.mag + a_ss.mag
    if s_res is None:
        dv = dv.rounded(1, dv.mag)                               # `ox = ux * a_vv`: 1 multiply
        # `(ux * vx + uy * vy + uz * vz) * a_sv + a_ss`: 3 products, 2 adds, 1 multiply, 1 add = 7
        ds = ds.rounded(7, ds_mag)
    else:
        r = q(v_res).view(lambda t: t.reshape(n, F, 3).transpose(0, 2, 1))
        sr = q(s_res).view(lambda t: t.reshape(n, F))
        dv = (dv + r).rounded(2, dv.mag + r.mag)                 # ... `ox += r.x`: multiply + add = 2
        ds = (ds + sr).rounded(8, ds_mag + sr.mag)               # ... `os += s_res[idx]`: 7 + 1 = 8
    return ds, dv.view(lambda t: t.transpose(0, 2, 1))


def gate_bwd(Ubuf, Vbuf, a, n, F, ld, u_col=0, v_col=0, g_ds=None, g_dv=None):
    """update_gate_bwd: gU, gVv [n, 3, F], ga [n, 3 F]; an absent upstream gradient is zero"""
    u, vv, a_vv, a_sv, _ = _gate_operands(Ubuf, Vbuf, a, n, F, ld, u_col, v_col)
    gs = _zeros(n, F) if g_ds is None else q(g_ds).view(lambda t: t.reshape(n, F))
    g = _zeros(n, 3, F) if g_dv is None else q(g_dv).view(lambda t: t.reshape(n, F, 3).transpose(0, 2, 1))
    inner_abs = (u.mag * vv.mag).sum(1)
    ga_vv = (g * u).sum(1).rounded(5, (g.mag * u.mag).sum(1))    # `gx * ux + gy * uy + gz * uz`: 3 products, 2 adds = 5
    # `inner = ux * vx + uy * vy + uz * vz` (5), `gs * inner` (1) = 6
    ga_sv = (gs * (u * vv).sum(1)).rounded(6, gs.mag * inner_abs)
    ga_ss = gs                                                   # `ga[c + 2 * F] = gs`: a copy
    cc = gs * a_sv                                               # `cc = gs * a_sv`: 1 multiply, counted below
    cb = cc.view(lambda t: t[:, None, :])
    av = a_vv.view(lambda t: t[:, None, :])
    gU = g * av + cb * vv
    gU = gU.rounded(3, g.mag * av.mag + cb.mag * vv.mag)         # `fmaf(gx, a_vv, cc * vx)`: cc, cc * vx, the fma = 3
    gVv = cb * u
    gVv = gVv.rounded(2, gVv.mag)                                # `cc * ux`: cc, the multiply = 2
    ga = Q(np.stack([ga_vv.val, ga_sv.val, ga_ss.val], 1).reshape(n, 3 * F), np.stack([ga_vv.err, ga_sv.err, ga_ss.err], 1).reshape(n, 3 * F))
    return gU, gVv, ga


# ------------------------------------------------------------------------------------------------ the products around them
def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def swish(z):
    """z * 1 / (1 + expf(-z)) (cgv_common.h act_fwd): expf within 1 ulp = 2 roundings (HIP's documented accuracy), the add,
    the division, the multiply = 5, all on one positive chain; |swish'| <= 1.1 carries the error of z."""
    z = q(z)
    val = z.val * _sigmoid(z.val)
    return Q(val, 1.1 * z.err).rounded(5, np.abs(val) + 1.1 * z.err)


def swish_prime(z):
    """s * (1 + z * (1 - s)) (act_bwd): s costs 4 and enters twice, `1 - s`, `z *`, `1 +`, `s *` one each = 12 over the
    terms s, s |z|, s |z| s; |swish''| <= 0.5 carries the error of z."""
    z = q(z)
    s = _sigmoid(z.val)
    return Q(s * (1.0 + z.val * (1.0 - s)), 0.5 * z.err).rounded(12, s * (1.0 + (np.abs(z.val) + z.err) * (1.0 + s)) + 0.5 * z.err)


def dense_fwd(x, W, b=None, extra=0):
    """x W^T (+ b) in fp32 in any order.  The longest path of any summation tree over K products is one product and K - 1
    adds = K roundings; + the bias add, + 1 for the activation-free epilogue's last add of partial sums:
    (K + 2) 2^-24 (sum |x| |W| + |b|), the any-order dot-product bound"""
    x, Wt = q(x), q(W).view(lambda t: t.T)
    K = x.shape[1]
    out, mag = _matmul(x, Wt), x.mag @ Wt.mag
    if b is not None:
        bq = q(b)
        out, mag = out + bq.view(lambda t: t[None, :]), mag + bq.mag[None, :]
    return out.rounded(K + 2 + extra, mag)


def dense_bwd_input(g, W, z=None, extra=0):
    """(g * swish'(z)) W, reduction over N: (N + 2) 2^-24 sum |g act'| |W| behind the operand's own error (act' and 1 multiply)"""
    g = q(g)
    if z is not None:
        g = times_swish_prime(g, z)
    N = g.shape[1]
    out = _matmul(g, W)
    return out.rounded(N + 2 + extra, g.mag @ q(W).mag)


def times_swish_prime(g, z):
    p = q(g) * swish_prime(z)
    return p.rounded(1, p.mag)                                   # `av.x *= act_bwd(...)` / `o[0] *= act_bwd(...)`: 1 multiply


def dense_wgrad(g, x):
    """gW = g^T x over M rows, gb = sum_m g.  More than 128 rows (and strips of 64 .. 96) run on the bf16 matrix path with
    split operands, whose documented loss is the dropped cross terms, below 2^-23 of a product (wgrad_gathered.hip): 2 more
    units per product than the fp32 tiles -- (M + 4) 2^-24 sum |g| |x| covers both."""
    g, x = q(g), q(x)
    M = g.shape[0]
    gt = g.view(lambda t: t.T)
    gW = _matmul(gt, x).rounded(M + 4, gt.mag @ x.mag)
    gb = g.sum(0).rounded(M + 2, g.mag.sum(0))
    return gW, gb


def bwd_input_norm_stack(gy, z, W, stack, Vv, n, F, ld, col, g_res=None, gVv_old=None, accumulate=0):
    """cgv_tile_linear_bwd_input_norm_stack: g_stack = (gy * act'(z)) W (z None: no activation), not stored, through
    norm_stack_bwd in the store epilogue -- the product's any-order bound carried through the epilogue's own count"""
    g_stack = dense_bwd_input(gy, W, z)
    return norm_stack_bwd(g_stack, Vv, stack, n, F, ld, col, g_res, gVv_old, accumulate)


# ------------------------------------------------------------------------------------------------ the whole block
PARAMS = ("u", "vw", "W0", "b0", "W1", "b1")


def block(s, v, params, residual, g_ds=None, g_dv=None, backward=True):
    """UpdateBlock forward (ds, dv; with ``residual`` s + ds, v + dv) and its analytic backward for the upstream gradients
    given (None: absent, i.e. zero), as the fused node runs them: one product with [u_mat; v_mat], the six launches above,
    s_dense.0 (Swish) and s_dense.1.  Returns a dict of Q with the bounds composed along the way."""
    n, F = np.shape(s)
    P = {k: q(params[k]) for k in PARAMS}
    Wuv = Q(np.concatenate([P["u"].val, P["vw"].val], 0))
    vt = rows_from_vec(v, n, F)
    UV = dense_fwd(vt, Wuv)                                                       # [3 n, 2 F]: U | Vv
    stack = norm_stack_fwd(s, UV, n, F, 2 * F, F)
    z0 = dense_fwd(stack, P["W0"], P["b0"])
    a0 = swish(z0)
    a = dense_fwd(a0, P["W1"], P["b1"])
    ds, dv = gate_fwd(UV, UV, a, n, F, 2 * F, 0, F, s if residual else None, v if residual else None)
    out = {"ds": ds, "dv": dv}
    if not backward or (g_ds is None and g_dv is None):
        return out
    gU, gVv, ga = gate_bwd(UV, UV, a, n, F, 2 * F, 0, F, g_ds, g_dv)
    g_z0 = times_swish_prime(dense_bwd_input(ga, P["W1"]), z0)
    g_stack = dense_bwd_input(g_z0, P["W0"])
    gUV = Q(np.concatenate([gU.val, gVv.val], 2).reshape(3 * n, 2 * F), np.concatenate([gU.err, gVv.err], 2).reshape(3 * n, 2 * F))
    g_s, gVv = norm_stack_bwd(g_stack, UV, stack, n, F, 2 * F, F, g_ds if residual else None, gUV, 1)
    gUV = Q(np.concatenate([gU.val, gVv.val], 2).reshape(3 * n, 2 * F), np.concatenate([gU.err, gVv.err], 2).reshape(3 * n, 2 * F))
    # (+ 1: the composition adds two F-deep products where the fused node runs one 2 F-deep one)
    g_vt = dense_bwd_input(gUV, Wuv, extra=1)
    out["g_s"], out["g_v"] = g_s, vec_from_rows(g_vt, n, F, g_dv if residual else None)
    gWuv, _ = dense_wgrad(gUV, vt)
    out["g_u"], out["g_vw"] = gWuv[:F], gWuv[F:]
    out["g_W1"], out["g_b1"] = dense_wgrad(ga, a0)
    out["g_W0"], out["g_b0"] = dense_wgrad(g_z0, stack)
    return out


# ------------------------------------------------------------------------------------------------ shared inputs
ELEMENTWISE_SHAPES = [(1, 4), (3, 20), (37, 7), (5, 52), (13, 36), (64, 128)]     # n F = 4 .. 8192; 259 and 260: the grid tail


def special_vv(Vv, n, F):
    """one Vv triple exactly 0, one of magnitude 1e-6, one of 1e3: whole nodes where there are three, else three columns"""
    scale = (0.0, 1e-6, 1e3)
    for i, sc in enumerate(scale):
        if n >= 3:
            Vv[i] = Vv[i] * np.float32(sc)
        else:
            Vv[0, :, i] = Vv[0, :, i] * np.float32(sc)
    return Vv


def elementwise_inputs(n, F, seed=0):
    """fp32 operands of the six launches: seeded normals, the special Vv triples, one gate column (an a_sv) zero"""
    g = np.random.default_rng(1000 * n + F + seed)
    rnd = lambda *sh: g.standard_normal(sh).astype(np.float32)
    d = dict(s=rnd(n, F), v=rnd(n, F, 3), U=rnd(n, 3, F), Vv=special_vv(rnd(n, 3, F), n, F), a=rnd(n, 3 * F), gstack=rnd(n, 2 * F),
             g_res=rnd(n, F), g_ds=rnd(n, F), g_dv=rnd(n, F, 3), old=rnd(n, 3, F))
    d["a"][:, F + 1] = 0.0
    return d


def as_buffers(U, Vv, n, F, ld):
    """(U buffer, u_col, Vv buffer, v_col): two [3 n, F] buffers (ld = F) or the halves of one [3 n, 2 F] (ld = 2 F)"""
    if ld == F:
        return U.reshape(3 * n, F).copy(), 0, Vv.reshape(3 * n, F).copy(), 0
    assert ld == 2 * F
    both = np.concatenate([U, Vv], 2).reshape(3 * n, 2 * F)
    return both, 0, both, F


# the fused epilogue: (id, M beads, F, the register-tile variant it lands on by shape)
EPILOGUE_SHAPES = [("r16w8-17-36", 17, 36), ("r16w8-33-36", 33, 36), ("r16w8-47-36", 47, 36), ("r16w8-17-128", 17, 128),
                   ("r16w8-33-128", 33, 128), ("r16w8-47-128", 47, 128), ("r32w8-1601-128", 1601, 128),
                   ("r32w4-4097-128", 4097, 128), ("r16w16-48-1024", 48, 1024)]


def epilogue_inputs(M, F, seed=0):
    """operands of cgv_tile_linear_bwd_input_norm_stack (N = F, K = 2 F, ld = 2 F): Vv with a zero and a 1e-6 node, the
    stack as norm_stack_fwd's fp32 kernel formula leaves it"""
    g = np.random.default_rng(7 * M + F + seed)
    rnd = lambda *sh: g.standard_normal(sh).astype(np.float32)
    d = dict(gy=rnd(M, F), z=rnd(M, F), W=(rnd(F, 2 * F) / np.float32(np.sqrt(F))), s=rnd(M, F), U=rnd(M, 3, F), g_res=rnd(M, F),
             old=rnd(M, 3, F))
    Vv = rnd(M, 3, F)
    Vv[0] = 0.0
    Vv[M - 1] = Vv[M - 1] * np.float32(1e-6)
    d["Vv"] = Vv
    d["stack"] = norm_stack_fwd_fp32(d["s"], Vv)
    return d


# ------------------------------------------------------------------------------------------------ the kernels' formulas in fp32
# numpy.float32 in the kernels' operation order (no contraction): what tests/test_update_cpu.py holds the bounds against
def norm_stack_fwd_fp32(s, Vv):
    e = np.float32(1e-10)
    x, y, z = Vv[:, 0], Vv[:, 1], Vv[:, 2]
    return np.concatenate([s, np.sqrt(((x * x + e) + (y * y + e)) + (z * z + e))], 1)


def norm_stack_bwd_fp32(gstack, Vv, stack, g_res=None, old=None):
    F = Vv.shape[2]
    g_s = gstack[:, :F] + g_res if g_res is not None else gstack[:, :F].copy()
    t = (gstack[:, F:] / stack[:, F:])[:, None, :]
    return g_s, (old + t * Vv if old is not None else t * Vv)


def gate_fwd_fp32(U, Vv, a, s_res=None, v_res=None):
    n, _, F = U.shape
    a3 = a.reshape(n, 3, F)
    dv = U * a3[:, 0][:, None, :]
    ds = ((U[:, 0] * Vv[:, 0] + U[:, 1] * Vv[:, 1]) + U[:, 2] * Vv[:, 2]) * a3[:, 1] + a3[:, 2]
    if s_res is not None:
        dv, ds = dv + v_res.transpose(0, 2, 1), ds + s_res
    return ds, dv.transpose(0, 2, 1)


def gate_bwd_fp32(U, Vv, a, g_ds=None, g_dv=None):
    n, _, F = U.shape
    a3 = a.reshape(n, 3, F)
    gs = np.zeros((n, F), np.float32) if g_ds is None else g_ds
    g = np.zeros((n, 3, F), np.float32) if g_dv is None else g_dv.transpose(0, 2, 1)
    inner = (U[:, 0] * Vv[:, 0] + U[:, 1] * Vv[:, 1]) + U[:, 2] * Vv[:, 2]
    cc = gs * a3[:, 1]
    ga = np.stack([(g[:, 0] * U[:, 0] + g[:, 1] * U[:, 1]) + g[:, 2] * U[:, 2], gs * inner, gs], 1).reshape(n, 3 * F)
    ccv = (cc[:, None, :] * Vv).astype(np.float64)
    gU = (g.astype(np.float64) * a3[:, 0][:, None, :].astype(np.float64) + ccv).astype(np.float32)     # fmaf: one rounding
    return gU, cc[:, None, :] * U, ga


def swish_prime_fp32(z):
    one = np.float32(1.0)
    s = one / (one + np.exp(-z))
    return s * (one + z * (one - s))
