"""Float64 reference, per-element error bounds, case tables and case runners for csrc/elementwise.hip -- TEST INFRASTRUCTURE ONLY.

Reference.  Every operation is a plain float64 torch expression of its mathematical definition on the CPU (F.binary_cross_entropy_with_logits, F.smooth_l1_loss,
F.l1_loss, F.mse_loss, KLDivLoss(batchmean) over log_softmax / softmax with autograd for its gradient, the textbook Adam update).  Nothing comes from
tests/fake_backend.py or from deepliif_amd (the enum values are restated in class L).  Operands are the values AS STORED (pre-rounded to the storage type), scalars
(alpha, lr, betas, eps, grad_scale ...) the fp32 values the C ABI receives.

Bound, per element:      |got - ref| <= e + u_store (|ref| + e) + tiny,      e = g(r) S  (+ what e's operands carry),  g(r) = r u / (1 - r u),  u = 2^-24
u_store = 2^-8 (bfloat16), 2^-11 (half), 0 (fp32: its roundings are the r counted below); tiny = 2^-126 (2^-24 for half: its subnormal spacing).  S is the sum of
the magnitudes of everything added, r the number of fp32 roundings on the path, counted from the source (a product of two 16-bit operands is exact in fp32:
P = 0 for 16-bit storage, 1 for fp32).  A sum of K addends in ANY order: g(K) S (the term of conv_ref); where the
kernel's summation tree is fixed and shorter than K (loss and KL sums), K is the number of roundings on its longest path, sum_len().  Floating-point contraction only removes roundings.

    op (kernel, file csrc/elementwise.hip unless noted)        r and S
    act_forward  RELU / NONE (common.h apply_act)              exact
                 LRELU  `0.2f * v`                             r = 2: 0.2f is not 0.2, the product; S = |ref|
                 TANH   `tanhf(v)`                             TANH_ULPS ulps of the result
                 SIGMOID `1.f / (1.f + __expf(-v))`            SIGMOID_ULPS ulps of the result (the whole expression is measured)
    act_backward RELU / NONE (act_grad_from_output)            exact (`g *= 1.f`, `g *= 0.f`)
                 LRELU  `y > 0.f ? 1.f : 0.2f`                 the choice is exact (compared with the one fp32 product); r = 2 against float64
                 TANH   `g *= 1.f - y * y`                     r = 2 + P: y y (P), 1 - y y, the product with g; S = |dy| (1 + y^2)
                 SIGMOID `g *= y * (1.f - y)`                  r = 3: 1 - y, y (1 - y), the product with g; S = |dy| |y| (1 + |y|)
    gate_forward, gate_backward dx  `v[k] *= a`                r = P; S = |ref|
    gate_backward dpsi  `part += gv * xv`, butterfly           K = Cp addends (+ P): g(Cp + P) sum_c |g x|; channels 1..7 exactly 0
    axpby        `alpha * va + beta * vb`                      r = 3 (two products, one sum), S = |alpha a| + |beta b|; without b: r = 1
    copy_channels                                              exact; accumulate `v += load1(d)`: r = 1 per call, and one store rounding per call
    upsample2    forward                                       exact; backward `v[k] += a[k]` four times from 0: g(3) sum |a|
    channel_sum  partial: per-thread, LDS rows; final: 8 lanes g(K + 1) sum |x|, K = pixels (+1: the fp32 cast of the double sum of the 8 lanes);
                 `out[c] + (float)a`                           accumulate: + u (|ref| + e)
    loss_kernel  inv_count `1.0f / (float)count`               1 rounding; gradient `g * gscale * inv_count`: r = r_g + 3
                 BCE    l = fmaxf(v, 0) - v t + log1pf(e)      g(2 + P) (|max(v, 0)| + |v t| + softplus) + SOFTPLUS_ULPS ulps of log1p(exp(-|v|))
                        g = sig - t, sig = 1 / (1 + e) | e / (1 + e), e = expf(-|v|):  sig (EXP_ULPS ulps of e relative + g(2)) + u |g|
                 MSE    d = v - t, l = d d, g = 2 d            l: r = 3 (d enters twice, the product), S = |l|; g: r = 1
                 LINEAR l = t v, g = t                         l: r = P (0 with a constant target of +-1); g exact
                 L1     l = |d|, g = sign(d)                   l: r = 1; g exact (the sign of a rounded difference is the sign of the difference)
                 SmoothL1 |d| < 1: 0.5 d d, else |d| - 0.5     l: r = 3, S = max(|l|, |d| + 0.5); g: r = 1 (d or +-1; the formulas agree at |d| = 1)
                 the mean: wave_sum, `red[0] + ...`, loss_final_kernel (double)      K = min(count, trips + 9), sum_len(): (sum e_l + g(K) sum (|l| + e_l)) / count, then
                 `(float)(tot * (double)inv_count) * out_scale`, `out[0] + v`        r = 3 (inv_count, the cast, out_scale) on |mean|; accumulate: + u |out|
    kldiv        zx += expf(x), zt += expf(t), a += et * (tv - xv)      every exponential EXP_ULPS ulps; a's term r = 1 + P; the three sums g(K) S each, K = sum_len(count)
                 `(float)(a / zt - log(zt) + log(zx)) * out_scale`      d KL = dA / Zt- + |A| dZt / (Zt Zt-) + dZt / Zt- + dZx / Zx-  (Z- = Z - dZ): ABSOLUTE,
                                                                        then r = 2 (cast, out_scale) on |KL| and the accumulate
                 gradient `gscale * (expf(x) * izx - expf(t) * izt)`    q (EXP + dZx / Zx- + g(3)) + p (likewise) + g(2) (q + p), times |gscale|
    adam_update  bc1 = 1.f - powf(b1, step) (host)             POW_ULPS (ulp of the power + u |bc1| where the difference rounds); bc2 likewise; sqrtf(bc2) on the host: half the relative error + u
                 step_size = lr / bc1                          relative error of bc1 + u
                 mi = b1 m + (1 - b1) gi, gi = g gscale        r = 4 (1 - b1, gi, its product, the sum), S = |b1 m| + |(1 - b1) gi|
                 vi = b2 v + (1 - b2) gi gi                    r = 6, S = b2 v + (1 - b2) gi^2
                 denom = sqrtf(vi) / bc2_sqrt + eps            sqrt(v) - sqrt(v - e_v) + SQRT_ULPS ulps, the quotient (bc2_sqrt's error + u), the sum (u)
                 p - step_size * (mi / denom)                  quotient, product, difference: one rounding each on their propagated operands
                 m, v, p additionally get 4 * 2^-149 for a product that underflows gradually

Device math functions.  ROCm installs no statement of the error of tanhf, expf, log1pf, sqrtf, powf or __expf (no HIP math document is part of the install), so
each constant below is MEASURED against the float64 reference by a dense sweep through the kernel that uses the function (tests/test_gpu_elementwise.py,
test_math_*; recorded in parity_errors_elementwise.json) and set to twice the recorded worst, rounded up to a power of two.  They are not derived.
    TANH_ULPS      act_forward(TANH), fp32, [-10, 10]
    SIGMOID_ULPS   act_forward(SIGMOID), fp32, [-30, 30]: __expf, the sum and the quotient together
    EXP_ULPS       expf over [-30, 1] through kldiv's gradient (one element holds the whole teacher mass, so the others read gscale expf(x) izx with izx taken from
                   the kernel's workspace): expf and one product rounding together
    SOFTPLUS_ULPS  log1pf(expf(-|v|)) over [-30, 0] through the BCE loss of single-element tensors (the mean of one element is the element)
    SQRT_ULPS      mi / (sqrtf(vi) / 0.5f) through adam_step with step_size = 1, p = 0, eps = 0, against the kernel's own stored m and v: sqrtf and one quotient
    POW_ULPS       1.f - powf(b, step) read from adam_hyper, steps 1 .. 100 000, in units of pow_unit() (one ulp of the power, plus the rounding of the
                   difference once the power is below 1/2): host code, the C library's powf
Recorded on the MI355X: 1.3488, 29.3606, 1.5503, 1.0963, 1.4410, 0.7331 ulps in this order (the constants below: 4, 64, 4, 4, 4, 2).

compare(): conv_ref.compare (the one pad_ref re-exports) on a 4-d view; its by-pixel and by-channel residues locate a stride or a second-trip error."""
import math

import torch
import torch.nn.functional as F

from pad_ref import compare as _compare4


class L:
    """the enum values of include/deepliif_hip.h, restated: this module imports nothing of the package (tests/test_elementwise_ref_host.py holds them to _lib)"""
    ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
    LOSS_BCE_LOGITS, LOSS_MSE, LOSS_SMOOTH_L1, LOSS_L1, LOSS_LINEAR = 0, 1, 2, 3, 4


U32 = 2.0 ** -24
U_STORE = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
ETA = 2.0 ** -147          # four gradual underflows
EW_THREADS = 8192 * 256          # EW_BLOCKS: the grid-stride loops take a second trip above this many work items
LOSS_THREADS = 512 * 256         # LOSS_BLOCKS
CS_BLOCKS = 256

# measured on the MI355X (see the module docstring): recorded worst -> constant
TANH_ULPS = 4.0          # recorded 1.3488
SIGMOID_ULPS = 64.0      # recorded 29.3606 (__expf: the argument's rounding grows with |v|; the worst is the negative tail)
EXP_ULPS = 4.0           # recorded 1.5503
SOFTPLUS_ULPS = 4.0      # recorded 1.0963
SQRT_ULPS = 4.0          # recorded 1.4410
POW_ULPS = 2.0           # recorded 0.7331
ACT_NAME = {L.ACT_NONE: 'none', L.ACT_RELU: 'relu', L.ACT_LRELU: 'lrelu', L.ACT_TANH: 'tanh', L.ACT_SIGMOID: 'sigmoid'}
LOSS_NAME = {L.LOSS_BCE_LOGITS: 'bce', L.LOSS_MSE: 'mse', L.LOSS_LINEAR: 'linear', L.LOSS_L1: 'l1', L.LOSS_SMOOTH_L1: 'smoothl1'}


SLACK = 1                # multiplier of every rounding count of the bounds; 1 = as derived


def g(k):
    k = SLACK * k
    return k * U32 / (1.0 - k * U32)


def sum_len(count):
    """the roundings on the longest path of loss_kernel's / kldiv_partial_kernel's fixed summation tree, never more than the number of addends: the per-thread
    grid-stride additions, the 6 levels of wave_sum, `red[0] + red[1] + red[2] + red[3]`; what follows is double (E64)"""
    return min(count, -(-count // LOSS_THREADS) + 6 + 3)


E64 = 600 * 2.0 ** -53          # the double sums of the 512 partials (and 64 slices) in the final kernels


def csum_rows(cp):
    """channel_sum_partial_kernel: pixels per block and trip (rows = 256 / tpp, tpp = min(Cp / 8, 256)); one trip of the whole grid covers CS_BLOCKS * rows pixels"""
    return 256 // min(cp // 8, 256)


def f32(v):
    """the fp32 value a C float argument receives"""
    return float(torch.tensor(v, dtype=torch.float32))


def P(dtype):
    return 1 if dtype == torch.float32 else 0


def tiny(dtype):
    return 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -126


def ulp32(x):
    """the spacing of fp32 at |x| (float64 tensor)"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def stored(ref, e, dtype, times=1):
    """the bound of a value computed with error e and rounded to the storage type `times` times"""
    b = e
    for _ in range(times):
        b = b + U_STORE[dtype] * (ref.abs() + b)
    return b + tiny(dtype)


def d64(t):
    return t.detach().double().cpu()


def compare(got, ref, bnd, axis='c'):
    """conv_ref.compare on NHWC; lower ranks become [1, 1, pixels, channels] (a vector runs along `axis`: 'c' channels, 'w' pixels)"""
    gv = got.detach().to('cpu', torch.float64)
    ref, bnd = torch.as_tensor(ref, dtype=torch.float64), torch.as_tensor(bnd, dtype=torch.float64)
    assert gv.numel() == ref.numel() == bnd.numel(), (gv.shape, ref.shape, bnd.shape)
    if gv.dim() != 4:
        last = gv.shape[-1] if gv.dim() >= 2 or (gv.dim() == 1 and axis == 'c') else 1
        shape = (1, 1, gv.numel() // max(last, 1), max(last, 1))
    else:
        shape = tuple(gv.shape)
    return _compare4(gv.reshape(shape), ref.reshape(shape), bnd.reshape(shape))


class Checker:
    """collects err / bound per output of one case and the exact assertions; done() asserts and files the ratios in `errlog`"""

    def __init__(self, tag, errlog):
        self.tag, self.errlog, self.ratios, self.reports = tag, errlog, {}, []

    def __call__(self, key, got, ref, bnd, axis='c'):
        worst, report = compare(got, ref, bnd, axis)
        self.ratios[key] = max(worst, self.ratios.get(key, 0.0))
        if report:
            self.reports.append(f'{key}: {report}')
        return worst

    def exact(self, key, got, want):
        got, want = got.detach().cpu(), want.detach().cpu()
        if not (got.shape == want.shape and torch.equal(got, want.to(got.dtype))):
            n = int((got != want.to(got.dtype)).sum()) if got.shape == want.shape else -1
            self.reports.append(f'{key}: not bit-exact ({n} of {got.numel()} elements differ)')
        self.ratios.setdefault(key + '(exact)', 0.0)

    def done(self):
        worst = max(self.ratios, key=self.ratios.get)
        self.errlog[self.tag] = {k: round(v, 4) for k, v in self.ratios.items()}
        print(f'{self.tag}: worst err/bound {self.ratios[worst]:.4f} ({worst}); ' + ' '.join(f'{k} {v:.3f}' for k, v in self.ratios.items()))
        assert self.ratios[worst] <= 1.0 and not self.reports, f'{self.tag}\n' + '\n'.join(self.reports)
        return self.ratios[worst]


# ------------------------------------------------------------------------------------------------ inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, dtype, scale=1.0):
    return (torch.randn(shape, generator=gen(seed)) * scale).to(dtype).float()


def tails(shape, seed, dtype, lo, hi, scale=2.0):
    """N(0, scale) with a quarter of the elements in the saturated tails +-[lo, hi], the first element exactly 0 and the next two +-hi"""
    ge = gen(seed)
    x = torch.randn(shape, generator=ge) * scale
    far = (lo + (hi - lo) * torch.rand(shape, generator=ge)) * (1 - 2 * (torch.rand(shape, generator=ge) < 0.5).float())
    x = torch.where(torch.rand(shape, generator=ge) < 0.25, far, x).clamp_(-hi, hi)
    flat = x.view(-1)
    flat[0] = 0.0
    if flat.numel() > 2:
        flat[1], flat[2] = hi, -hi
    return x.to(dtype).float()


TAILS = {L.ACT_SIGMOID: (9.0, 30.0), L.ACT_TANH: (5.0, 10.0)}


def act_input(shape, seed, dtype, act):
    lo, hi = TAILS.get(act, (5.0, 10.0))
    return tails(shape, seed, dtype, lo, hi)


class Arena:
    """places the operands of one call: dense tensors, or (view) channel slices of wider buffers -- a different width and offset per operand, so every pixel
    stride differs from Cp and from the others.  check() asserts that the buffers kept their sentinel outside the slices and that no input was written."""
    LAYOUT = [(lambda cp: 2 * cp, 8), (lambda cp: cp + 8, 8), (lambda cp: 4 * cp, 16), (lambda cp: 3 * cp, 0), (lambda cp: cp + 24, 16), (lambda cp: 5 * cp, 8)]

    def __init__(self, dev, dtype, view):
        self.dev, self.dtype, self.view, self.bufs, self.k = dev, dtype, view, [], 0

    def _place(self, shape, fill, src):
        cp = shape[-1]
        if not self.view:
            t = torch.full(shape, fill, dtype=self.dtype, device=self.dev)
            if src is not None:
                t.copy_(src.to(self.dtype))
                self.bufs.append((None, t, 0, cp, fill, src))
            return t
        width, lo = self.LAYOUT[self.k % len(self.LAYOUT)]
        self.k += 1
        buf = torch.full(tuple(shape[:-1]) + (width(cp),), fill, dtype=self.dtype, device=self.dev)
        v = buf[..., lo:lo + cp]
        if src is not None:
            v.copy_(src.to(self.dtype))
        self.bufs.append((buf, v, lo, cp, fill, src))
        return v

    def put(self, src, fill=7.0):
        return self._place(tuple(src.shape), fill, src)

    def out(self, shape, fill=-3.0):
        return self._place(tuple(shape), fill, None)

    def check(self, chk):
        for i, (buf, v, lo, cp, fill, src) in enumerate(self.bufs):
            if buf is not None:
                keep = torch.ones(buf.shape[-1], dtype=torch.bool)
                keep[lo:lo + cp] = False
                if not bool((buf.cpu()[..., keep] == fill).all()):
                    chk.reports.append(f'operand {i}: the wider buffer changed outside its channel slice')
            if src is not None and not torch.equal(v.cpu(), src.to(self.dtype)):
                chk.reports.append(f'operand {i}: an input was written to')


# ------------------------------------------------------------------------------------------------ references (value, bound of the COMPUTED value; stored() adds the store)
def act64(act, x):
    if act == L.ACT_RELU:
        return torch.relu(x)
    if act == L.ACT_LRELU:
        return F.leaky_relu(x, 0.2)
    if act == L.ACT_TANH:
        return torch.tanh(x)
    if act == L.ACT_SIGMOID:
        return torch.sigmoid(x)
    return x.clone()


def act_forward_ref(act, x):
    x = d64(x)
    ref = act64(act, x)
    if act == L.ACT_LRELU:
        e = torch.where(x > 0, torch.zeros_like(x), g(2) * ref.abs())
    elif act == L.ACT_TANH:
        e = TANH_ULPS * ulp32(ref)
    elif act == L.ACT_SIGMOID:
        e = SIGMOID_ULPS * ulp32(ref)
    else:
        e = torch.zeros_like(x)
    return ref, e


def act_backward_ref(act, dy, y, dtype):
    dy, y = d64(dy), d64(y)
    if act == L.ACT_RELU:
        return dy * (y > 0), torch.zeros_like(dy)
    if act == L.ACT_LRELU:
        ref = torch.where(y > 0, dy, 0.2 * dy)
        return ref, torch.where(y > 0, torch.zeros_like(dy), g(2) * ref.abs())
    if act == L.ACT_TANH:
        return dy * (1 - y * y), g(2 + P(dtype)) * dy.abs() * (1 + y * y)
    if act == L.ACT_SIGMOID:
        return dy * y * (1 - y), g(3) * dy.abs() * y.abs() * (1 + y.abs())
    return dy.clone(), torch.zeros_like(dy)


def gate_ref(x, psi, dtype):
    ref = d64(x) * d64(psi)[..., :1]
    return ref, g(P(dtype)) * ref.abs()


def gate_dpsi_ref(gr, x, dtype):
    prod = d64(gr) * d64(x)
    cp = prod.shape[-1]
    ref = torch.zeros(prod.shape[:-1] + (8,), dtype=torch.float64)
    ref[..., 0] = prod.sum(-1)
    e = torch.zeros_like(ref)
    e[..., 0] = g(cp + P(dtype)) * prod.abs().sum(-1)
    return ref, e


def axpby_ref(alpha, a, beta, b):
    if b is None:
        ref = alpha * d64(a)
        return ref, g(1) * ref.abs()
    ta, tb = alpha * d64(a), beta * d64(b)
    return ta + tb, g(3) * (ta.abs() + tb.abs())


def upsample2_ref(src, backward):
    s = d64(src)
    if not backward:
        return s.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2), None
    n, h2, w2, c = s.shape
    v = s.view(n, h2 // 2, 2, w2 // 2, 2, c)
    return v.sum(dim=(2, 4)), g(3) * v.abs().sum(dim=(2, 4))


def channel_sum_ref(x, C, old, accumulate):
    xv = d64(x)[..., :C].reshape(-1, C)
    K = xv.shape[0]
    s, S = xv.sum(0), xv.abs().sum(0)
    e = g(K + 1) * S
    if not accumulate:
        return s, e + tiny(torch.float32)
    ref = d64(old) + s
    return ref, e + U32 * (ref.abs() + e) + tiny(torch.float32)


def loss_ref(kind, x, target, tconst, C, dtype, gscale=1.0, out_scale=1.0, old=None):
    """(loss value, its bound, gradient over the C real channels, its bound before the store).  old: the value accumulated onto (None: overwrite)"""
    v = d64(x)[..., :C].clone().requires_grad_(True)
    t = d64(target)[..., :C] if target is not None else torch.full_like(v, tconst)
    count = v.numel()
    vd, ad = v.detach(), (v.detach() - t).abs()
    if kind == L.LOSS_BCE_LOGITS:
        mean = F.binary_cross_entropy_with_logits(v, t)
        sp = torch.log1p(torch.exp(-vd.abs()))
        l_abs = vd.clamp_min(0) + (vd * t).abs() + sp
        e_l = g(2 + P(dtype)) * l_abs + SOFTPLUS_ULPS * ulp32(sp)
        sig = torch.sigmoid(vd)
        e_g = sig * (2 * EXP_ULPS * U32 + g(2)) + U32 * (sig - t).abs()
    elif kind == L.LOSS_MSE:
        mean = F.mse_loss(v, t)
        l_abs = ad * ad
        e_l, e_g = g(3) * l_abs, g(1) * 2 * ad
    elif kind == L.LOSS_LINEAR:
        mean = (t * v).mean()
        l_abs = (t * vd).abs()
        e_l, e_g = g(P(dtype) if target is not None else 0) * l_abs, torch.zeros_like(vd)
    elif kind == L.LOSS_L1:
        mean = F.l1_loss(v, t)
        l_abs = ad
        e_l, e_g = g(1) * ad, torch.zeros_like(vd)
    else:
        mean = F.smooth_l1_loss(v, t, beta=1.0)
        l_abs = torch.where(ad < 1, 0.5 * ad * ad, ad - 0.5)
        e_l = g(3) * torch.maximum(l_abs, torch.where(ad < 1, l_abs, ad + 0.5))
        e_g = g(1) * ad.clamp_max(1.0)
    mean.backward()
    grad = v.grad * gscale
    # g * gscale * inv_count: three more roundings (gscale's product, inv_count itself, its product)
    b_grad = (e_g + g(3) * (v.grad.abs() * count + e_g)) * abs(gscale) / count
    mean = mean.detach()
    e_mean = (float(e_l.sum()) + (g(sum_len(count)) + E64) * float((l_abs + e_l).sum())) / count
    val = float(mean) * out_scale
    e_val = abs(out_scale) * (e_mean + g(3) * (abs(float(mean)) + e_mean))
    if old is not None:
        val = float(old) + val
        e_val = e_val + U32 * (abs(val) + e_val)
    return val, e_val + tiny(torch.float32), grad, b_grad


def kldiv_ref(x, t, C, dtype, gscale=1.0, out_scale=1.0, old=None):
    """(KL value, its ABSOLUTE bound, gradient over the real channels, its bound before the store)"""
    shape = d64(x)[..., :C].shape
    xv = d64(x)[..., :C].reshape(1, 1, -1).clone().requires_grad_(True)
    tv = d64(t)[..., :C].reshape(1, 1, -1)
    kl = torch.nn.KLDivLoss(reduction='batchmean')(torch.log_softmax(xv, -1), torch.softmax(tv, -1))
    kl.backward()
    K = xv.numel()
    ke = 2 * EXP_ULPS * U32
    xd = xv.detach()
    ex, et = torch.exp(xd), torch.exp(tv)
    Zx, Zt = float(ex.sum()), float(et.sum())
    a = et * (tv - xd)
    A, Aabs = float(a.sum()), float(a.abs().sum())
    gK = g(sum_len(K)) + E64
    dZx = ke * Zx + gK * Zx * (1 + ke)
    dZt = ke * Zt + gK * Zt * (1 + ke)
    ea = ke + g(1 + P(dtype))
    dA = ea * Aabs + gK * Aabs * (1 + ea)
    assert dZx < Zx / 2 and dZt < Zt / 2
    Zxm, Ztm = Zx - dZx, Zt - dZt
    dkl = dA / Ztm + abs(A) * dZt / (Zt * Ztm) + dZt / Ztm + dZx / Zxm
    klv = float(kl.detach())
    val = klv * out_scale
    e_val = abs(out_scale) * (dkl + g(2) * (abs(klv) + dkl))
    if old is not None:
        val = float(old) + val
        e_val = e_val + U32 * (abs(val) + e_val)
    q, p = ex / Zx, et / Zt
    b = q * (ke + dZx / Zxm + g(3)) + p * (ke + dZt / Ztm + g(3))
    b = (b + g(2) * (q + p + b)) * abs(gscale)
    return val, e_val + tiny(torch.float32), (xv.grad * gscale).reshape(shape), b.reshape(shape)


def pow_bc(b, step):
    """(1 - b^step, its bound) as dl_adam_step computes it: powf on the host, one subtraction"""
    pw = b ** step
    bc = 1.0 - pw
    return bc, POW_ULPS * pow_unit(pw, bc)


def pow_unit(pw, bc):
    """the unit POW_ULPS counts: one ulp of the power plus the rounding of the difference (exact while the power is at least 1/2)"""
    return float(ulp32(torch.tensor(pw, dtype=torch.float64))) + (U32 * bc if pw < 0.5 else 0.0)


def adam_ref(p, gr, m, v, lr, b1, b2, eps, step, gscale):
    """one textbook Adam step from the given fp32 state in float64: {'p', 'm', 'v'} and their bounds"""
    p, gr, m, v = d64(p), d64(gr), d64(m), d64(v)
    gi = gr * gscale
    tm, tg = b1 * m, (1 - b1) * gi
    mi = tm + tg
    e_m = g(4) * (tm.abs() + tg.abs()) + ETA
    vi = b2 * v + (1 - b2) * gi * gi
    e_v = g(6) * vi + ETA
    bc1, e_bc1 = pow_bc(b1, step)
    bc2, e_bc2 = pow_bc(b2, step)
    r1, r2 = e_bc1 / (bc1 - e_bc1), e_bc2 / (bc2 - e_bc2)
    rs = r2 / 2 * (1 + r2) + U32 * (1 + r2)           # sqrtf(bc2) on the host: IEEE
    rss = r1 + U32 * (1 + r1)                       # lr / bc1
    s = vi.sqrt()
    e_s = s - (vi - e_v).clamp_min(0).sqrt() + SQRT_ULPS * ulp32(s + (vi + e_v).sqrt() - s)
    bs = math.sqrt(bc2)
    h = s / bs
    e_h = (e_s + (s + e_s) * (rs / (1 - rs) + U32)) / bs
    den = h + eps
    e_den = e_h + U32 * (den + e_h)
    assert bool((e_den < den).all()), 'the bound of the denominator passes the denominator (eps = 0 and v = 0?)'
    denm = den - e_den
    q = mi / den
    e_q = e_m / denm + mi.abs() * e_den / (den * denm)
    e_q = e_q + U32 * (q.abs() + e_q)
    ss = lr / bc1
    upd = ss * q
    e_u = ss * (1 + rss) * e_q + ss * rss * q.abs()
    e_u = e_u + U32 * (upd.abs() + e_u)
    pn = p - upd
    e_p = e_u + U32 * (pn.abs() + e_u) + ETA
    return {'p': pn, 'm': mi, 'v': vi}, {'p': e_p, 'm': e_m, 'v': e_v}


# ------------------------------------------------------------------------------------------------ case tables
VEC_SHAPES = [(2, 9, 11, 8), (1, 7, 5, 512), (3, 1, 1, 16)]
VIEW_SHAPE = (2, 9, 11, 32)          # every operand a slice of a wider buffer: pixel strides 64 / 40 / 128 / 96 ...
BIG_SHAPE = (1, 164, 200, 512)       # 32 800 pixels x 64 vectors = 2 099 200 > EW_THREADS: the second trip of the grid-stride loop
ACTS = [L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH, L.ACT_SIGMOID, L.ACT_NONE]
BIG_ACT = L.ACT_LRELU
assert BIG_SHAPE[1] * BIG_SHAPE[2] * (BIG_SHAPE[3] // 8) == 2099200 > EW_THREADS

# copy_channels: (shape of the source, source width, s_c0, destination width, d_c0, C)
COPY_CASES = [((2, 9, 11), 24, 3, 40, 13, 5), ((1, 7, 5), 16, 1, 8, 2, 6), ((3, 1, 1), 8, 0, 16, 7, 8), ((1, 1025, 1024), 8, 2, 8, 1, 3)]
assert 1025 * 1024 * 3 > EW_THREADS

# gate_backward: (pixels as N, H, W), Cp
GATE_BWD_CASES = [((1, 1, 1), 8), ((1, 1, 7), 8), ((1, 7, 9), 8), ((2, 9, 11), 16), ((2, 9, 11), 64), ((1, 7, 5), 512), ((1, 17, 241), 512),
                  ((1, 164, 200), 512)]          # the last row: 2 099 200 work items, the second trip of gate_bwd_kernel's `rounded` loop
assert 17 * 241 == 4097 and 164 * 200 * 64 > EW_THREADS

# channel_sum: (Cp, pixels as (N, H, W), real C, strided view)
CSUM_CASES = [(8, (1, 65537, 1), 3, False), (8, (1, 5, 1), 8, False), (32, (2, 9, 11), 20, False), (512, (1, 41, 25), 512, False), (512, (1, 3, 1), 500, False),
              (64, (2, 175, 200), 64, True)]
assert 41 * 25 == 1025 and 2 * 175 * 200 == 70000

LOSS_KINDS = [L.LOSS_BCE_LOGITS, L.LOSS_MSE, L.LOSS_LINEAR, L.LOSS_L1, L.LOSS_SMOOTH_L1]
LOSS_SHAPES = [((2, 30, 30), 1), ((2, 30, 30), 3), ((2, 30, 30), 8), ((1, 1, 1), 1), ((1, 1, 1), 3), ((2, 181, 182), 3)]
assert 2 * 181 * 182 * 3 == 197652 > LOSS_THREADS
LOSS_CONST = {L.LOSS_BCE_LOGITS: 1.0, L.LOSS_MSE: 1.0, L.LOSS_LINEAR: -1.0, L.LOSS_L1: 0.0, L.LOSS_SMOOTH_L1: 0.0}

KL_SHAPES = [((2, 64, 64), 3), ((1, 37, 53), 3), ((1, 16, 16), 1), ((2, 181, 182), 3), ((8, 512, 512), 3)]

ADAM_N = [1, 255, 256, 257, 100003, 2097153]
ADAM_STEPS = [1, 2, 1000, 100000]
ADAM_GSCALE = [1.0, 1.0 / 1024]
ADAM_BETAS = [(0.5, 0.999), (0.9, 0.999)]
assert ADAM_N[-1] > EW_THREADS


# ------------------------------------------------------------------------------------------------ case runners (be: a backend; dev: where its tensors live)
def run_act_forward(be, dev, chk, shape, dtype, act, view=False, sync=lambda: None):
    x = act_input(shape, 11, dtype, act)
    ar = Arena(dev, dtype, view)
    xd, yd = ar.put(x), ar.out(shape)
    be.act_forward(act, xd, yd)
    sync()
    ref, e = act_forward_ref(act, x)
    key = 'fwd-' + ACT_NAME[act]
    if act in (L.ACT_RELU, L.ACT_NONE):
        chk.exact(key, yd, ref.to(dtype))
    else:
        chk(key, yd, ref, stored(ref, e, dtype))
    ar.check(chk)


def act_backward_inputs(shape, dtype, act):
    x = act_input(shape, 12, dtype, act)
    y = act64(act, x.double()).to(dtype).float()          # the stored output of the forward: after a ReLU about half of it is exactly 0
    if act == L.ACT_LRELU:
        y.view(-1)[::7] = 0.0          # y == 0 takes the slope
    return rnd(shape, 13, dtype), y


def run_act_backward(be, dev, chk, shape, dtype, act, view=False, sync=lambda: None):
    dy, y = act_backward_inputs(shape, dtype, act)
    if act == L.ACT_RELU:
        assert 0.3 < float((y == 0).float().mean()) < 0.7
    ar = Arena(dev, dtype, view)
    dyd, yd, dxd = ar.put(dy), ar.put(y), ar.out(shape)
    be.act_backward(act, dyd, yd, dxd)
    sync()
    ref, e = act_backward_ref(act, dy, y, dtype)
    key = 'bwd-' + ACT_NAME[act]
    if act in (L.ACT_RELU, L.ACT_NONE):
        chk.exact(key, dxd, ref.to(dtype))
    else:
        chk(key, dxd, ref, stored(ref, e, dtype))
    if act == L.ACT_LRELU:          # the choice of the factor: y > 0 passes dy, everything else is the ONE fp32 product with 0.2f
        chk.exact(key + '-factor', dxd, torch.where(y > 0, dy, dy * torch.tensor(0.2, dtype=torch.float32)).to(dtype))
    ar.check(chk)


def gate_inputs(shape, dtype):
    psi = torch.zeros(tuple(shape[:3]) + (8,))
    psi[..., 0] = torch.rand(shape[:3], generator=gen(23)).to(dtype).float()
    psi[..., 1:] = 5.0          # only channel 0 is the gate: the rest must not be read
    return rnd(shape, 21, dtype), rnd(shape, 22, dtype), psi


def run_gate_forward(be, dev, chk, shape, dtype, view=False, sync=lambda: None):
    x, _, psi = gate_inputs(shape, dtype)
    ar = Arena(dev, dtype, view)
    xd, pd, od = ar.put(x), ar.put(psi), ar.out(shape)
    be.gate_forward(xd, pd, od)
    sync()
    ref, e = gate_ref(x, psi, dtype)
    chk('gate', od, ref, stored(ref, e, dtype))
    ar.check(chk)


def run_gate_backward(be, dev, chk, shape, dtype, view=False, with_dx=True, sync=lambda: None):
    x, gr, psi = gate_inputs(shape, dtype)
    ar = Arena(dev, dtype, view)
    gd, xd, pd = ar.put(gr), ar.put(x), ar.put(psi)
    dxd = ar.out(shape) if with_dx else None
    dpd = ar.out(tuple(shape[:3]) + (8,))
    be.gate_backward(gd, xd, pd, dxd, dpd)
    sync()
    if with_dx:
        ref, e = gate_ref(gr, psi, dtype)
        chk('gate-dx', dxd, ref, stored(ref, e, dtype))
    ref, e = gate_dpsi_ref(gr, x, dtype)
    chk('dpsi', dpd, ref, stored(ref, e, dtype))
    chk.exact('dpsi[1:]', dpd[..., 1:], torch.zeros(tuple(shape[:3]) + (7,)))
    ar.check(chk)


def run_axpby(be, dev, chk, shape, dtype, with_b, view=False, sync=lambda: None):
    a, b = rnd(shape, 31, dtype), rnd(shape, 32, dtype, 3.0)
    alpha, beta = f32(0.7), f32(-1.3)
    ar = Arena(dev, dtype, view)
    ad = ar.put(a)
    bd = ar.put(b) if with_b else None
    od = ar.out(shape)
    be.axpby(alpha, ad, beta, bd, od)
    sync()
    ref, e = axpby_ref(alpha, a, beta, b if with_b else None)
    chk('axpby' if with_b else 'scale', od, ref, stored(ref, e, dtype))
    ar.check(chk)


def run_upsample2(be, dev, chk, shape, dtype, backward, view=False, sync=lambda: None):
    n, h, w, cp = shape          # the SMALL tensor
    big = (n, 2 * h, 2 * w, cp)
    src = rnd(big if backward else shape, 41, dtype)
    ar = Arena(dev, dtype, view)
    sd, dd = ar.put(src), ar.out(shape if backward else big)
    be.upsample2(sd, dd, backward=backward)
    sync()
    ref, e = upsample2_ref(src, backward)
    if backward:
        chk('upsample2-bwd', dd, ref, stored(ref, e, dtype))
    else:
        chk.exact('upsample2-fwd', dd, ref.to(dtype))
    ar.check(chk)


def run_copy_channels(be, dev, chk, case, dtype, accumulate, sync=lambda: None):
    pix, sw, s0, dw, d0, C = case
    src = rnd(pix + (sw,), 51, dtype)
    dst0 = rnd(pix + (dw,), 52, dtype)
    sd, dd = src.to(dtype).to(dev, copy=True), dst0.to(dtype).to(dev, copy=True)
    times = 2 if accumulate else 1          # accumulate twice: the second call reads back what the first one rounded
    for _ in range(times):
        be.copy_channels(sd, s0, dd, d0, C, accumulate=accumulate)
    sync()
    keep = torch.ones(dw, dtype=torch.bool)
    keep[d0:d0 + C] = False
    chk.exact('copy-rest', dd[..., keep], dst0[..., keep].to(dtype))
    chk.exact('copy-src', sd, src.to(dtype))
    s = d64(src)[..., s0:s0 + C]
    if not accumulate:
        chk.exact('copy', dd[..., d0:d0 + C], s.to(dtype))
        return
    d = d64(dst0)[..., d0:d0 + C]
    r1 = d + s
    b1 = stored(r1, g(1) * r1.abs(), dtype)
    ref = r1 + s
    chk('copy-acc', dd[..., d0:d0 + C], ref, stored(ref, b1 + g(1) * (ref.abs() + b1), dtype))


def run_channel_sum(be, dev, chk, case, dtype, accumulate, mean=0.0, spread=1.0, sync=lambda: None):
    cp, pix, C, view = case
    x = torch.full(pix + (cp,), 3.0)          # the padding channels hold a value: they must not reach the real ones
    x[..., :C] = (torch.randn(pix + (C,), generator=gen(61)) * spread + mean).to(dtype).float()
    sgn = (1 - 2 * (torch.arange(C) % 2)).float()
    x[0, -1, -1, :C] = mean + 3.0 * spread * sgn          # the last pixel weighs 3: an off-by-one at the end of a single trip shows
    npix, stride = pix[0] * pix[1] * pix[2], CS_BLOCKS * csum_rows(cp)
    if npix > stride:
        # Later trips of the grid: the bound is g(K + 1) sum |x|, so a trip that is dropped (or taken twice) shows only if its SIGNED sum outweighs that.
        # Every pixel past the first trip holds mean + sgn_c amp (1 .. 1.25), amp chosen so that the smallest later trip weighs 8 times the bound.
        flat = x.view(npix, cp)
        m, n_last = npix - stride, npix - (npix - 1) // stride * stride
        ku = 8 * g(npix + 1)
        s_body = float(flat[:stride, :C].abs().sum(0).max())
        assert ku * 1.25 * m / n_last < 1, 'the later trips cannot outweigh the bound at this shape'
        amp = max(spread, ku * s_body / (n_last * (1 - ku * 1.25 * m / n_last)))
        flat[stride:, :C] = mean + sgn * amp * (1 + 0.25 * torch.rand(m, C, generator=gen(63)))
    x = x.to(dtype).float()
    ar = Arena(dev, dtype, view)
    xd = ar.put(x)
    old = torch.randn(C, generator=gen(62))
    out = old.to(dev, copy=True)
    be.channel_sum(xd, C, out, accumulate)
    sync()
    ref, b = channel_sum_ref(x, C, old, accumulate)
    chk('csum', out, ref, b)
    ar.check(chk)


def loss_inputs(kind, pix, C, dtype, with_target):
    """x, target (or None) as [N, H, W, 8]; the padding channels hold 0.5 (they must not be read)"""
    shape = pix + (C,)
    ge = gen(71)
    us = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}[dtype]
    if kind == L.LOSS_BCE_LOGITS:
        x = tails(shape, 72, dtype, 10.0, 30.0, 3.0)
        t = torch.rand(shape, generator=ge).to(dtype).float()
    else:
        t = (torch.rand(shape, generator=ge) * 2 - 1).to(dtype).float() if with_target else torch.full(shape, LOSS_CONST[kind])
        x = (t + torch.randn(shape, generator=ge)).to(dtype).float()
        if kind in (L.LOSS_L1, L.LOSS_SMOOTH_L1):
            sel = torch.rand(shape, generator=ge)
            x = torch.where(sel < 0.25, t, x)          # x == target exactly: sign(0) = 0
            near = (sel >= 0.25) & (sel < 0.5)          # |d| within one storage ulp of 1, with x, target and d = x - target all exact
            sg = 1 - 2 * (torch.rand(shape, generator=ge) < 0.5).float()
            d = sg * torch.tensor([1 - us, 1.0, 1 + 2 * us])[torch.randint(0, 3, shape, generator=ge)]
            if with_target:
                tn = -0.5 * sg
                t = torch.where(near, tn, t)
            x = torch.where(near, (t.double() + d.double()).float(), x)
            dd = (x.double() - t.double())[near]
            assert torch.equal(x.to(dtype).float(), x) and torch.equal(dd.float().double(), dd) and bool(((dd.abs() - 1).abs() <= 2 * us).all())
    xp = torch.full(pix + (8,), 0.5)
    xp[..., :C] = x
    if not with_target:
        return xp, None
    tp = torch.full(pix + (8,), 0.5)
    tp[..., :C] = t
    return xp, tp


def run_loss(be, dev, chk, kind, pix, C, dtype, with_target, view=False, with_grad=True, gscale=1.0, out_scale=1.0, accumulate=False, sync=lambda: None):
    x, t = loss_inputs(kind, pix, C, dtype, with_target)
    gscale, out_scale = f32(gscale), f32(out_scale)
    ar = Arena(dev, dtype, view)
    xd = ar.put(x)
    td = ar.put(t) if t is not None else None
    gd = ar.out(pix + (8,), fill=9.0) if with_grad else None
    old = torch.tensor([0.625])
    out = old.to(dev, copy=True)
    be.loss(kind, xd, td, LOSS_CONST[kind], C, out, gd, gscale, out_scale=out_scale, accumulate=accumulate)
    sync()
    val, e_val, grad, b_grad = loss_ref(kind, x, t, LOSS_CONST[kind], C, dtype, gscale, out_scale, old[0] if accumulate else None)
    key = LOSS_NAME[kind]
    chk(key, out, torch.tensor([val]), torch.tensor([e_val]))
    if with_grad:
        chk(key + '-grad', gd[..., :C], grad, stored(grad, b_grad, dtype))
        if C < 8:
            chk.exact(key + '-grad-padding', gd[..., C:], torch.zeros(pix + (8 - C,)))
        if kind == L.LOSS_L1:          # +-(1 * gscale) * inv_count in fp32, or exactly 0
            inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(x[..., :C].numel()), dtype=torch.float32)
            sgn = torch.sign(x[..., :C].double() - (t[..., :C].double() if t is not None else LOSS_CONST[kind])).float()
            chk.exact(key + '-grad-sign', gd[..., :C], (sgn * torch.tensor(gscale, dtype=torch.float32) * inv).to(dtype))
    ar.check(chk)


def kl_inputs(pix, C, dtype, near):
    ge = gen(81)
    x0 = torch.tanh(torch.randn(pix + (C,), generator=ge)).to(dtype).float()
    if near:          # the student next to the teacher: t = x + delta, 0 <= delta <= 2^-7 (a non-zero mean: A / Zt does not vanish), both representable
        t0 = (x0 + torch.rand(pix + (C,), generator=ge) * 2.0 ** -7).clamp_(-1, 1).to(dtype).float()
    else:
        t0 = (torch.rand(pix + (C,), generator=ge) * 2 - 1).to(dtype).float()
    x = torch.full(pix + (8,), 3.0)
    t = torch.full(pix + (8,), -2.0)          # garbage in the padding channels must not matter
    x[..., :C], t[..., :C] = x0, t0
    assert float(x0.abs().max()) <= 1 and float(t0.abs().max()) <= 1
    return x, t


def run_kldiv(be, dev, chk, pix, C, dtype, near, view=False, with_grad=True, gscale=1.0, out_scale=1.0, accumulate=False, sync=lambda: None):
    x, t = kl_inputs(pix, C, dtype, near)
    gscale, out_scale = f32(gscale), f32(out_scale)
    ar = Arena(dev, dtype, view)
    xd, td = ar.put(x), ar.put(t)
    gd = ar.out(pix + (8,), fill=9.0) if with_grad else None
    old = torch.tensor([0.625])
    out = old.to(dev, copy=True)
    be.kldiv(xd, td, C, out, gd, gscale, out_scale=out_scale, accumulate=accumulate)
    sync()
    val, e_val, grad, b_grad = kldiv_ref(x, t, C, dtype, gscale, out_scale, old[0] if accumulate else None)
    chk('kl', out, torch.tensor([val]), torch.tensor([e_val]))
    if with_grad:
        chk('kl-grad', gd[..., :C], grad, stored(grad, b_grad, dtype))
        if C < 8:
            chk.exact('kl-grad-padding', gd[..., C:], torch.zeros(pix + (8 - C,)))
    ar.check(chk)
    return val, e_val


def adam_state(n, seed=91, tiny_v=True):
    """p, g, m, v (fp32).  A quarter of the elements: g = 0 on m = v = 0 (p must not move); an eighth: v near the smallest normal fp32 with a gradient that small"""
    ge = gen(seed)
    p = torch.randn(n, generator=ge) * 0.02
    gr = torch.randn(n, generator=ge)
    m = torch.randn(n, generator=ge) * 0.1
    v = torch.rand(n, generator=ge) * 0.01
    idx = torch.arange(n)
    zero = idx % 4 == 1
    gr[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
    if tiny_v:
        tv = idx % 8 == 2
        v[tv] = 2.0 ** -125 * (1 + 7 * torch.rand(n, generator=ge)[tv])
        gr[tv] = 2.0 ** -48 * (1 + 3 * torch.rand(n, generator=ge)[tv])          # times grad_scale 2^-10: gi ~ 2^-58, (1 - b2) gi^2 stays normal
        m[tv] = gr[tv] * 0.5
    return p, gr, m, v, zero


def run_adam_step(be, dev, chk, n, step, gscale, betas, dev_variant=True, sync=lambda: None):
    p, gr, m, v, zero = adam_state(n)
    lr, b1, b2, eps, gscale = f32(2e-4), f32(betas[0]), f32(betas[1]), f32(1e-8), f32(gscale)
    pd, gd, md, vd = (t.to(dev, copy=True) for t in (p, gr, m, v))
    be.adam_step(pd, gd, md, vd, lr, b1, b2, eps, step, gscale)
    sync()
    ref, bnd = adam_ref(p, gr, m, v, lr, b1, b2, eps, step, gscale)
    for k, got in (('p', pd), ('m', md), ('v', vd)):
        chk(f'adam-{k}', got, ref[k], bnd[k] + 0 * ref[k], axis='w')
    chk.exact('adam-p(g=0,m=v=0)', pd[zero.to(dev)], p[zero])
    chk.exact('adam-grad', gd, gr)
    if dev_variant:
        hyper = torch.zeros(8)
        be.adam_hyper(lr, b1, b2, eps, step, gscale, hyper)
        p2, m2, v2 = (t.to(dev, copy=True) for t in (p, m, v))
        be.adam_step_dev(p2, gd, m2, v2, hyper.to(dev))
        sync()
        for k, a, b in (('p', p2, pd), ('m', m2, md), ('v', v2, vd)):
            chk.exact(f'adam_step_dev-{k}', a, b)


def run_adam_trajectory(be, dev, chk, n, betas, gscale, sync=lambda: None):
    """three steps; each step's reference starts from the kernel's own previous state, so the errors do not compound"""
    p, gr, m, v, _ = adam_state(n, tiny_v=False)
    lr, b1, b2, eps, gscale = f32(2e-4), f32(betas[0]), f32(betas[1]), f32(1e-8), f32(gscale)
    pd, md, vd = (t.to(dev, copy=True) for t in (p, m, v))
    for step in (1, 2, 3):
        gs = torch.randn(n, generator=gen(100 + step)) / gscale
        p0, m0, v0 = pd.cpu().clone(), md.cpu().clone(), vd.cpu().clone()
        be.adam_step(pd, gs.to(dev), md, vd, lr, b1, b2, eps, step, gscale)
        sync()
        ref, bnd = adam_ref(p0, gs, m0, v0, lr, b1, b2, eps, step, gscale)
        for k, got in (('p', pd), ('m', md), ('v', vd)):
            chk(f'step{step}-{k}', got, ref[k], bnd[k] + 0 * ref[k], axis='w')
