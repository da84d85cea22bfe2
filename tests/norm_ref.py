"""Float64 reference, per-element error bound and a locating comparer for the normalisation kernels (csrc/norm.hip) -- TEST INFRASTRUCTURE ONLY.

Reference: written from the definition in float64 on the CPU (two-pass mean and biased variance; instance scope per (n, c), batch scope per c), not from
tests/fake_backend.py.  Operands are pre-rounded to the storage type by the caller, so kernel and reference see identical inputs; the backward takes the
REFERENCE's statistics rounded to fp32 (Reference.stats32) on both sides, so its bound does not carry the forward's error.

    forward    rstd = (var + eps)^-1/2, scale = gamma rstd, shift = beta - mean scale, nv = y scale + shift, z = act(nv) + residual
               running_mean = (1 - m) running_mean + m mean, running_var likewise with the UNBIASED variance; m < 0 leaves both untouched
    backward   dn = dz act'(nv), xh = (y - mean) rstd, c1 = mean(dn), c2 = mean(dn xh), dy = gamma rstd (dn - c1 - xh c2),
               dgamma += sum dn xh, dbeta += sum dn, dy_chansum += sum dy (real channels)

Bound.  u = 2^-24, g(k) = k u / (1 - k u): k fp32 roundings on one path (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 4.2).
A sum of fp32 terms t_i added in ANY order whose longest path has L additions is off by at most g(L) sum|t_i|.  L is read off the kernels (geometry() restates
make_geom, the tpp / rows rule and apply_grid):
    statistics and backward reductions (norm_partial_kernel, norm_chunk_sum_kernel)
        L = ceil(ppc / rows)  per-thread additions  +  min(rows, ppc)  the serial LDS reduction (thread rows without a pixel add exact zeros, and they
            come last)  +  ceil(ceil(nchunks / 32) / 4) + 2  one chunk lane: four independent accumulators, then two levels joining them
    channel sums of dy (norm_bwd_apply_kernel, norm_bias_final_kernel: eight accumulators per lane, three levels)
        Lb = ceil(HW / (blocks rows)) + min(rows, HW) + ceil(ceil(blocks N / 32) / 8) + 3
Everything behind the chunk lanes is fp64 (a relative (40 + N) 2^-53 is allowed for it) and is cast to fp32 once.  `slack` multiplies L and Lb only.
With A1 = E|y|, A2 = E y^2 over the group (an image, or the batch) and mu, var its float64 statistics:
    d mu   = g(L + 1) A1                                   (+1: the chunk sums are stored as fp32)
    d var  = g(L + 2) A2 + 2 |mu| d mu + d mu^2            (the kernel's variance is E y^2 - mu^2; +1 more for the square; clamped at 0 like the kernel's)
    mean   : d mu + u |mu|
    rstd   : max((max(var - d var, 0) + eps)^-1/2 - rstd, rstd - (var + d var + eps)^-1/2) + u rstd
             = d var / (2 (var + eps)) rstd to first order -- the exact propagation stays finite (and honest) where d var > var + eps
    scale  : |gamma| d rstd + u |scale|
    shift  : d(mean scale) + 2 u |mean scale| + u |beta|   (product and difference: one rounding each, fused or not)
    nv     : |y - mean| d scale + |scale| d mean + the shift's roundings + u (2 |y scale| + |shift|)      (shift is built from the same scale: mean d scale cancels)
    z      : d nv (ReLU / LeakyReLU are 1-Lipschitz; LeakyReLU: + 2 u |act|, the fp32 slope and its product) + u |z| (the residual add) + us |z| (the store)
d var / (var + eps) carries A2 / (var + eps): the bound widens by itself on channels whose mean is large against their spread -- that is the error the
documented algorithm (fp32 sums of y and y^2) can really make, not a tolerance.
    running: m d mean (d unbiased var) + g(4) ((1 - m) |old| + m |new|)
Backward, with exact fp32 statistics on both sides (sums over the group, E = mean over it):
    mask   : the kernel's nv = fl(y scale + shift) is off by <= u (2 |y scale| + |shift|) < 2^-13 <= |nv| (asserted: KINK / 2), so both sides take the same branch
    c1     : g(L + 3) E|dn| + u |c1|               (LeakyReLU's 0.2f dz: 2 roundings; the fp32 cast of the chunk sum)
    c2     : g(L + 6) E|dn xh| + u |c2|            (dn (y - mean) rstd: 3 more)
    dgamma : g(L + 6) sum|dn xh| + u (|old| + |new|), dbeta: g(L + 3) sum|dn| + u (|old| + |new|)
    xh     : u (|y rstd| + |mean rstd| + |xh|)     (the kernel evaluates y rstd - mean rstd)
    t = dn - c1 - xh c2 : d dn + d c1 + |xh| d c2 + d xh |c2| + g(3) (|dn| + |c1| + |xh c2|)
    dy     : |gamma rstd| (d t + 2 u |t|) + us |dy|
    chansum: sum (d dy without the store) + g(Lb + 1) sum|dy| + u (|old| + |new|)
us = 2^-8 (bfloat16), 2^-11 (IEEE half; + 2^-25 absolute for its subnormals), 2^-24 (fp32).  No constant here is fitted to a measurement.

compare(): worst err / bound and, on a violation, WHERE: by image, chunk index, pixel mod rows, first / last pixel of a chunk, 8-channel column, channel mod 8."""
import torch

from deepliif_amd import _lib as L

U32 = 2.0 ** -24
U_STORE = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
KINK = 2.0 ** -12
BIAS_PART_ROWS = 2048          # csrc/norm.hip kBiasPartRows
EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # dl_norm_desc.eps is a float: the reference sees the same value


def g(k):
    return k * U32 / (1.0 - k * U32)


def cdiv(a, b):
    return -(-a // b)


# ---- the kernels' geometry, restated
def geometry(N, HW, Cp):
    """make_geom, the tpp / rows rule of the streaming kernels and apply_grid (csrc/norm.hip)"""
    want, maxc = cdiv(1024, N), cdiv(HW, 64)
    nch = max(1, min(want, maxc))
    ppc = cdiv(HW, nch)
    nch = cdiv(HW, ppc)
    cvec = Cp // 8
    col_tpp = [min(cvec - (col // 256) * 256, 256) for col in range(cvec)]
    col_rows = [256 // t for t in col_tpp]
    rows0 = 256 // min(cvec, 256)
    blocks = max(1, min(cdiv(HW, rows0 * 16), max(1, BIAS_PART_ROWS // N)))
    return {'N': N, 'HW': HW, 'Cp': Cp, 'nchunks': nch, 'ppc': ppc, 'col_tpp': col_tpp, 'col_rows': col_rows, 'blocks': blocks}


def ws_floats(N, HW, Cp, ext_nchunks=0):
    """what dl_norm_ws_floats has to cover: partials | chunk sums, c1, c2 | one row of Cp bias partials per apply block (+ the 64 floats of slack it always had)"""
    ge = geometry(N, HW, Cp)
    return N * max(ge['nchunks'], ext_nchunks) * 2 * Cp + 4 * N * Cp + ge['blocks'] * N * Cp


def sum_lengths(ge, slack=1):
    """(L, Lb) per channel [Cp]: additions on the longest fp32 path of the statistics / of the channel sums of dy"""
    rows = torch.tensor(ge['col_rows'], dtype=torch.float64).repeat_interleave(8)
    Ls = torch.ceil(ge['ppc'] / rows) + rows.clamp(max=ge['ppc']) + cdiv(cdiv(ge['nchunks'], 32), 4) + 2
    Lb = torch.ceil(ge['HW'] / (ge['blocks'] * rows)) + rows.clamp(max=ge['HW']) + cdiv(cdiv(ge['blocks'] * ge['N'], 32), 8) + 3
    return slack * Ls, slack * Lb


def _act(act, v):
    if act == L.ACT_RELU:
        return torch.relu(v)
    if act == L.ACT_LRELU:
        return torch.where(v > 0, v, 0.2 * v)
    assert act == L.ACT_NONE, act
    return v


def _pad(v, C, Cp, fill):
    out = torch.zeros(Cp, dtype=torch.float64)
    out[:C] = fill if v is None else v.double().cpu()
    return out


class Reference:
    """float64 statistics of one (y, scope, affine); forward() / running() / backward() derive the variants together with their per-element bounds"""

    def __init__(self, y, C, scope, gamma=None, beta=None, eps=EPS, slack=1, sum_len=None):
        self.y = y.detach().double().cpu()
        self.N, self.H, self.W, self.Cp = self.y.shape
        self.C, self.scope, self.eps = C, scope, eps
        self.HW = self.H * self.W
        self.ge = geometry(self.N, self.HW, self.Cp)
        self.L, self.Lb = sum_lengths(self.ge, slack)
        if sum_len is not None:          # statistics from another producer (a convolution's epilogue): its own longest path
            self.L = torch.full_like(self.L, float(slack * sum_len))
        self.dims = (0, 1, 2) if scope == L.NORM_BATCH else (1, 2)
        self.cnt = self.HW * (self.N if scope == L.NORM_BATCH else 1)
        N, Cp = self.N, self.Cp
        red = lambda t: t.mean(dim=self.dims, keepdim=True).reshape(-1, Cp).expand(N, Cp).contiguous()
        self.red = red
        self.mean = red(self.y)
        self.var = red((self.y - self.mean.view(N, 1, 1, Cp)) ** 2)
        self.A1, self.A2 = red(self.y.abs()), red(self.y * self.y)
        self.rstd = (self.var + eps) ** -0.5
        self.gamma, self.beta = _pad(gamma, C, Cp, 1.0), _pad(beta, C, Cp, 0.0)
        self.scale = self.gamma * self.rstd
        self.shift = self.beta - self.mean * self.scale
        # what the backward reads on both sides: the fp32 statistics
        self.stats32 = torch.stack([self.mean, self.rstd, self.scale, self.shift]).float()
        self._stat_bounds()

    # ---- forward
    def _stat_bounds(self):
        e64 = (40 + self.N) * 2.0 ** -53
        dmu = (g(self.L + 1) + e64) * self.A1
        self.dvar = (g(self.L + 2) + 4 * e64) * self.A2 + 2 * self.mean.abs() * dmu + dmu * dmu
        self.b_mean = dmu + U32 * (self.mean.abs() + dmu)
        hi = ((self.var - self.dvar).clamp_min(0) + self.eps) ** -0.5 - self.rstd
        lo = self.rstd - (self.var + self.dvar + self.eps) ** -0.5
        drs = torch.maximum(hi, lo)
        self.b_rstd = drs + (U32 + e64) * (self.rstd + drs)
        self.b_scale = self.gamma.abs() * self.b_rstd + U32 * self.gamma.abs() * (self.rstd + self.b_rstd)
        P = self.mean.abs() * self.scale.abs()
        dP = self.mean.abs() * self.b_scale + self.b_mean * (self.scale.abs() + self.b_scale)
        self.r_shift = 2 * U32 * (P + dP) + U32 * self.beta.abs()          # the shift's own roundings
        self.b_shift = dP + self.r_shift
        # how much the variance term widens the bound: E y^2 / (var + eps)
        self.conditioning = self.A2 / (self.var + self.eps)

    def stat_bounds(self):
        return {'mean': self.b_mean, 'rstd': self.b_rstd, 'scale': self.b_scale, 'shift': self.b_shift}

    def stats(self):
        return {'mean': self.mean, 'rstd': self.rstd, 'scale': self.scale, 'shift': self.shift}

    def nv(self):
        N, Cp = self.N, self.Cp
        return self.y * self.scale.view(N, 1, 1, Cp) + self.shift.view(N, 1, 1, Cp)

    def near_kink(self):
        """elements of the real channels whose normalised value is closer to the activation's kink than KINK"""
        m = self.nv().abs() < KINK
        m[..., self.C:] = False
        return m

    def forward(self, act, residual, dtype):
        """(z, bound of z)"""
        N, Cp = self.N, self.Cp
        v = lambda t: t.view(N, 1, 1, Cp)
        ya = self.y.abs()
        nv = self.nv()
        # the errors of scale and shift are not independent: shift = beta - mean scale with the SAME scale, so what reaches nv is (y - mean) d scale + scale d mean
        # (+ the roundings of the shift itself); |y| d scale + d shift would count mean d scale twice, and it is the largest term on an ill-conditioned channel
        b = (self.y - v(self.mean)).abs() * v(self.b_scale) + v(self.b_mean * (self.scale.abs() + self.b_scale) + self.r_shift)
        b += U32 * (2 * ya * v(self.scale.abs() + self.b_scale) + v(self.shift.abs() + self.b_shift))
        del ya
        z = _act(act, nv)
        del nv
        if act == L.ACT_LRELU:
            b += 2 * U32 * z.abs()
        if residual is not None:
            z = z + residual.detach().double().cpu()
            b += U32 * (z.abs() + b)
        b += U_STORE[dtype] * (z.abs() + b)
        if dtype == torch.float16:
            b += 2.0 ** -25
        return z, b

    def running(self, rm0, rv0, momentum):
        """((running_mean, running_var), their bounds) after one forward; momentum is the fp32 value the kernel sees"""
        C = self.C
        rm0, rv0 = rm0.double().cpu(), rv0.double().cpu()
        if momentum < 0:
            return (rm0, rv0), (torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64))
        assert self.scope == L.NORM_BATCH
        m = float(torch.tensor(momentum, dtype=torch.float32))
        mu, var = self.mean[0, :C], self.var[0, :C]
        k = self.cnt / (self.cnt - 1.0) if self.cnt > 1 else 1.0
        unb = var * k
        rm, rv = (1 - m) * rm0 + m * mu, (1 - m) * rv0 + m * unb
        b_unb = self.dvar[0, :C] * k + U32 * (unb + self.dvar[0, :C] * k)
        b_rm = m * self.b_mean[0, :C] + g(4) * ((1 - m) * rm0.abs() + m * (mu.abs() + self.b_mean[0, :C]))
        b_rv = m * b_unb + g(4) * ((1 - m) * rv0.abs() + m * (unb + b_unb))
        return (rm, rv), (b_rm, b_rv)

    # ---- backward (statistics: stats32 on both sides)
    def backward(self, act, dz, dtype, dgamma0=None, dbeta0=None, chansum0=None, exact_stats=False):
        """{'dy', 'dgamma', 'dbeta', 'chansum', 'c1', 'c2'} and the same keys' bounds.  dgamma0 / dbeta0 / chansum0: the values accumulated onto ([C]).
        exact_stats: the float64 statistics in place of stats32 (the definition itself, for the comparison with autograd; the bounds assume stats32)"""
        N, Cp, C = self.N, self.Cp, self.C
        v = lambda t: t.view(N, 1, 1, Cp)
        mean, rstd, scale, shift = (self.mean, self.rstd, self.scale, self.shift) if exact_stats else (self.stats32[i].double() for i in range(4))
        dzv = dz.detach().double().cpu()
        nv = self.y * v(scale) + v(shift)
        b_nv = U32 * (2 * (self.y * v(scale)).abs() + v(shift.abs()))
        real = torch.zeros(Cp, dtype=torch.bool)
        real[:C] = True
        if act != L.ACT_NONE and not exact_stats:
            # (KINK / 2 on either side: repair_kink measured with the float64 statistics, these are their fp32 roundings)
            assert bool(((nv.abs() >= KINK / 2) | ~real).all()), 'an element sits on the kink of the activation: repair the inputs (repair_kink)'
            assert float(b_nv.max()) < KINK / 2
        del b_nv
        if act == L.ACT_RELU:
            dn = dzv * (nv > 0)
            b_dn = None
        elif act == L.ACT_LRELU:
            dn = torch.where(nv > 0, dzv, 0.2 * dzv)
            b_dn = torch.where(nv > 0, torch.zeros_like(dn), 2 * U32 * dn.abs())
        else:
            dn, b_dn = dzv, None
        del nv, dzv
        xh = (self.y - v(mean)) * v(rstd)
        red = self.red
        c1, c2 = red(dn), red(dn * xh)
        e64 = (40 + N) * 2.0 ** -53
        E1, E2 = red(dn.abs()), red((dn * xh).abs())
        b_c1 = (g(self.L + 3) + e64) * E1 + U32 * c1.abs()
        b_c2 = (g(self.L + 6) + e64) * E2 + U32 * c2.abs()
        sdn, sdx = dn.sum(dim=(0, 1, 2)), (dn * xh).sum(dim=(0, 1, 2))
        Sdn, Sdx = dn.abs().sum(dim=(0, 1, 2)), (dn * xh).abs().sum(dim=(0, 1, 2))
        out, bnd = {'c1': c1, 'c2': c2}, {'c1': b_c1, 'c2': b_c2}
        for key, s, S, k, old in (('dgamma', sdx, Sdx, 6, dgamma0), ('dbeta', sdn, Sdn, 3, dbeta0)):
            old = torch.zeros(C, dtype=torch.float64) if old is None else old.double().cpu()
            out[key] = old + s[:C]
            bnd[key] = (g(self.L[:C] + k) + e64) * S[:C] + U32 * (old.abs() + 2 * s[:C].abs())
        gr =self.gamma * rstd          # [N, Cp]; gamma is 0 on the padding channels
        t = dn - v(c1) - xh * v(c2)
        ya = self.y.abs()
        b_xh = U32 * (ya * v(rstd) + v((mean * rstd).abs()) + xh.abs())
        del ya
        b_t = v(b_c1) + xh.abs() * v(b_c2) + b_xh * v(c2.abs() + b_c2) + g(3) * (dn.abs() + v(c1.abs() + b_c1) + (xh.abs() + b_xh) * v(c2.abs() + b_c2))
        del b_xh, xh
        if b_dn is not None:
            b_t += b_dn
        dy = v(gr) * t
        b_dy = v(gr.abs()) * (b_t + 2 * U32 * (t.abs() + b_t))
        del t, b_t, dn
        cs0 = torch.zeros(C, dtype=torch.float64) if chansum0 is None else chansum0.double().cpu()
        s, S = dy.sum(dim=(0, 1, 2))[:C], dy.abs().sum(dim=(0, 1, 2))[:C]
        out['chansum'] = cs0 + s
        bnd['chansum'] = b_dy.sum(dim=(0, 1, 2))[:C] + g(self.Lb[:C] + 1) * (S + b_dy.sum(dim=(0, 1, 2))[:C]) + U32 * (cs0.abs() + 2 * s.abs()) + e64 * S
        b_dy += U_STORE[dtype] * (dy.abs() + b_dy)
        if dtype == torch.float16:
            b_dy += 2.0 ** -25
        out['dy'], bnd['dy'] = dy, b_dy
        return out, bnd


def reference(y, C, scope, act, gamma=None, beta=None, residual=None, dz=None, dtype=torch.float32, running=None, momentum=-1.0, dgamma0=None, dbeta0=None,
              chansum0=None, slack=1, exact_stats=False):
    """everything at once: (values, bounds), two dicts with the keys mean, rstd, scale, shift, z (+ running_mean, running_var when `running` = (rm0, rv0))
    (+ dy, dgamma, dbeta, chansum, c1, c2 when dz is given).  The sweeps use the Reference object directly to share the statistics between activations."""
    r = Reference(y, C, scope, gamma, beta, slack=slack)
    val, bnd = dict(r.stats()), dict(r.stat_bounds())
    val['z'], bnd['z'] = r.forward(act, residual, dtype)
    if running is not None:
        (val['running_mean'], val['running_var']), (bnd['running_mean'], bnd['running_var']) = r.running(running[0], running[1], momentum)
    if dz is not None:
        bv, bb = r.backward(act, dz, dtype, dgamma0, dbeta0, chansum0, exact_stats)
        val.update(bv)
        bnd.update(bb)
    return val, bnd


def bound(*args, **kw):
    """the bounds alone (see the module docstring for the derivation)"""
    return reference(*args, **kw)[1]


# ---- the ReLU kink
def repair_kink(y, C, scope, gamma, beta, dtype, rounds=5):
    """The float64 reference and the fp32 kernel may disagree on the sign of a normalised value that is nearly zero, and act' jumps there.  No element is
    left out of the comparison: the INPUT is moved instead.  Elements with |y scale + shift| < KINK get another value of the storage type (half a standard
    deviation up or down), until none is left (the statistics move a little with every repair).  Returns (y, elements still near the kink)."""
    y = y.clone()
    left = 0
    for _ in range(rounds + 1):
        r = Reference(y, C, scope, gamma, beta)
        m = r.near_kink()
        left = int(m.sum())
        if left == 0:
            break
        # alternately up and down within a channel: the repair itself must not move the mean by more than one element's worth
        sign = 1.0 - 2.0 * (m.view(-1, r.Cp).cumsum(0) % 2).view(m.shape)
        step = (0.5 / r.rstd).view(r.N, 1, 1, r.Cp) * sign
        moved = (y.double() + step).to(dtype).to(y.dtype)
        y = torch.where(m, moved, y)
    return y, left


# ---- the comparer
def _hist(idx, n_show=8):
    v, c = torch.unique(idx, return_counts=True)
    order = torch.argsort(c, descending=True)[:n_show]
    more = '' if v.numel() <= n_show else f' (+{v.numel() - n_show} more values)'
    return '{' + ', '.join(f'{int(v[i])}: {int(c[i])}' for i in order) + '}' + more


def compare(got, ref, bnd, ge=None):
    """got: tensor of any dtype / device; ref, bnd: float64 of the same shape -- NHWC, or [N, Cp] / [C] for the per-channel results.  Returns (worst err /
    bound, report); report is '' when every element is in bound.  An element whose bound is 0 (a padding channel) must be exact.  ge: geometry() for the report."""
    gv = got.detach().to('cpu', torch.float64)
    assert gv.shape == ref.shape == bnd.shape, (gv.shape, ref.shape, bnd.shape)
    err = (gv - ref).abs_()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)          # 0 / 0 -> 0, x / 0 -> inf, NaN stays
    ratio = ratio.nan_to_num_(nan=float('inf'), posinf=float('inf'))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst <= 1.0:
        return worst, ''
    bad = ratio > 1.0
    nbad = int(bad.sum())
    idx = bad.nonzero(as_tuple=True)
    lines = [f'{nbad} of {bad.numel()} elements out of bound ({100.0 * nbad / bad.numel():.3g} %), worst err/bound {worst:.4g}',
             f'  first: index {tuple(int(i[0]) for i in idx)}: got {float(gv[bad][0])!r}, reference {float(ref[bad][0])!r}, bound {float(bnd[bad][0]):.3g}']
    c = idx[-1]
    if gv.dim() >= 2:
        lines.append(f'  by image            {_hist(idx[0])}')
    if gv.dim() == 4 and ge is not None:
        p = idx[1] * gv.shape[2] + idx[2]
        ppc = ge['ppc']
        rows = torch.tensor(ge['col_rows'])[c // 8]
        inchunk = p % ppc
        last = torch.minimum((p // ppc + 1) * ppc, torch.tensor(ge['HW'])) - 1
        lines += [f"  chunks of {ppc} pixels ({ge['nchunks']} per image); apply grid {ge['blocks']} x {ge['N']}",
                  f'  by chunk index      {_hist(p // ppc)}',
                  f'  by pixel mod rows   {_hist(p % rows)}',
                  f'  first pixel of a chunk: {int((inchunk == 0).sum())}, last pixel of a chunk: {int((p == last).sum())}']
    lines += [f'  by 8-channel column {_hist(c // 8)}', f'  by channel mod 8    {_hist(c % 8)}']
    return worst, '\n'.join(lines)


def split_decode(buf):
    """the strict policy's split copy (fp32-shaped buffer, [8 bf16 hi | 8 bf16 lo] per eight channels) -> (hi, lo) as float64 NHWC"""
    n, h, w, cp = buf.shape
    raw = buf.detach().cpu().contiguous().view(torch.bfloat16).view(n, h, w, cp // 8, 16)
    return raw[..., :8].reshape(n, h, w, cp).double(), raw[..., 8:].reshape(n, h, w, cp).double()


# ---- the sweep's geometry rows and inputs (tests/test_gpu_norm.py on the GPU, tests/test_norm_ref_host.py on the emulation)
SWEEP = [
    # (N, H, W, Cp), C real         what it reaches
    ((2, 5, 7, 8), 3),              # one chunk, tpp = 1, rows = 256 with fewer pixels than rows
    ((2, 33, 31, 8), 3),            # 16 chunks, the last one short (63 of 64)
    ((1, 96, 96, 16), 12),          # 144 chunks: the unrolled chunk loop once, plus a tail
    ((1, 256, 256, 8), 3),          # 1024 chunks: the maximum, eight trips of the unrolled loop
    ((3, 40, 36, 24), 20),          # Cp = 24: tpp = 3, rows = 85, one idle thread, ragged last chunk (54 of 63)
    ((3, 150, 150, 24), 24),        # Cp = 24, 341 chunks of 66 pixels, the last 60
    ((5, 48, 40, 128), 100),        # odd batch, C < Cp inside the last columns
    ((8, 64, 64, 256), 256),        # 256 bias partials: the unrolled loop of norm_bias_final_kernel
    ((8, 128, 128, 64), 64),        # want-limited chunks (ppc = 128), the benched ratio of batch to map
    ((2, 12, 10, 2048), 2048),      # tpp = 256, rows = 1
    ((1, 4, 4, 4096), 4096),        # second trip of the cbase loop
    ((3, 7, 5, 256), 256),          # kept from test_norm_forward_backward
]
# what the rows above are there for: (nchunks, ppc, pixels of the last chunk, rows of column 0, apply blocks) -- fails when make_geom / apply_grid change under the table
SWEEP_GEOMETRY = [(1, 35, 35, 256, 1), (16, 64, 63, 256, 1), (144, 64, 64, 128, 5), (1024, 64, 64, 256, 16), (23, 63, 54, 85, 2), (341, 66, 60, 85, 17),
                  (30, 64, 64, 16, 8), (64, 64, 64, 8, 32), (128, 128, 128, 32, 32), (2, 60, 60, 1, 8), (1, 16, 16, 1, 1), (1, 35, 35, 8, 1)]


def case_id(case):
    (n, h, w, cp), c = case
    return f'n{n}h{h}w{w}cp{cp}c{c}'


def check_sweep_geometry():
    for ((n, h, w, cp), _), want in zip(SWEEP, SWEEP_GEOMETRY):
        ge = geometry(n, h * w, cp)
        got = (ge['nchunks'], ge['ppc'], h * w - (ge['nchunks'] - 1) * ge['ppc'], ge['col_rows'][0], ge['blocks'])
        assert got == want, ((n, h, w, cp), got, want)


def _randn(shape, seed, dtype, scale=1.0, mean=0.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + mean).to(dtype).float()


def make_inputs(case, scope, dtype, affine=None, mean=0.3, spread=1.7, repair=True):
    """y, residual, dz (fp32 tensors holding values of the storage type, padding channels 0), gamma, beta (None without an affine; default: batch scope has
    one) and the count of elements left near the activation's kink.  The last pixel of every image holds +-3: an off-by-one at the end of the last chunk moves
    the statistics by 3 / HW, which at 65 536 pixels would otherwise hide inside the summation bound."""
    (n, h, w, cp), c = case
    affine = (scope == L.NORM_BATCH) if affine is None else affine
    t = {}
    for k, (seed, sc, mu) in {'y': (1, spread, mean), 'res': (2, 1.0, 0.0), 'dz': (3, 1.0, 0.0)}.items():
        t[k] = torch.zeros(n, h, w, cp)
        t[k][..., :c] = _randn((n, h, w, c), seed, dtype, sc, mu)
    t['y'][:, -1, -1, :c] = (mean + spread * 3.0 * (1 - 2 * (torch.arange(c) % 2))).to(dtype).float()
    t['gamma'] = (1 + 0.1 * torch.randn(c, generator=torch.Generator().manual_seed(4))) if affine else None
    t['beta'] = (0.1 * torch.randn(c, generator=torch.Generator().manual_seed(5))) if affine else None
    t['near_kink'] = 0
    if repair:
        t['y'], t['near_kink'] = repair_kink(t['y'], c, scope, t['gamma'], t['beta'], dtype)
    return t
