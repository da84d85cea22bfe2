"""tests/norm_ref.py checked on the CPU, without the kernels:
  * the float64 reference against torch's instance_norm / batch_norm and their autograd gradients;
  * its bound against a numpy fp32 emulation of the kernels' documented summation order (per-thread sums, the serial row reduction, the chunk lanes with their
    four accumulators, fp64 behind them; the channel sums of dy through the apply grid and norm_bias_final_kernel's eight accumulators) on every geometry row
    of the GPU sweep -- the bound has to hold -- and against eleven subtly wrong variants of that emulation -- the bound has to reject each of them on every
    row where the mutated path is live;
  * the workspace contract of dl_norm_ws_floats (the library loads without a GPU; nothing here launches anything)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from deepliif_amd import _lib as L

f32 = np.float32
ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU)
SCOPES = (L.NORM_INSTANCE, L.NORM_BATCH)
SCOPE_NAME = {L.NORM_INSTANCE: 'instance', L.NORM_BATCH: 'batch'}


# ------------------------------------------------------------------------------------------------ the reference against torch
@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'affine'])
@pytest.mark.parametrize('scope', SCOPES, ids=SCOPE_NAME.get)
def test_reference_equals_torch_in_float64(scope, affine):
    n, h, w, c, cp = 3, 6, 5, 11, 16
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    for act in ACTS:
        for with_res in (False, True):
            y = torch.zeros(n, h, w, cp, dtype=torch.float64)
            y[..., :c] = rnd(n, h, w, c) * 1.7 + 0.3
            res = torch.zeros_like(y)
            res[..., :c] = rnd(n, h, w, c)
            dz = torch.zeros_like(y)
            dz[..., :c] = rnd(n, h, w, c)
            gamma, beta = (1 + 0.1 * rnd(c), 0.1 * rnd(c)) if affine else (None, None)
            rm0, rv0, cs0, dg0, db0 = rnd(c), rnd(c).abs() + 0.5, rnd(c), rnd(c), rnd(c)
            momentum = float(torch.tensor(0.1, dtype=torch.float32))
            running = (rm0, rv0) if scope == L.NORM_BATCH else None
            val, _ = R.reference(y, c, scope, act, gamma, beta, res if with_res else None, dz, torch.float32, running, momentum if running else -1.0,
                                 dg0 if affine else None, db0 if affine else None, cs0, exact_stats=True)
            x = y[..., :c].permute(0, 3, 1, 2).clone().requires_grad_(True)
            gt, bt = (gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)) if affine else (None, None)
            rm, rv = rm0.clone(), rv0.clone()
            if scope == L.NORM_BATCH:
                nrm = F.batch_norm(x, rm, rv, gt, bt, True, momentum, R.EPS)
            else:
                nrm = F.instance_norm(x, None, None, gt, bt, True, 0.0, R.EPS)
            a = {L.ACT_NONE: lambda v: v, L.ACT_RELU: torch.relu, L.ACT_LRELU: lambda v: F.leaky_relu(v, 0.2)}[act](nrm)
            zt = a + res[..., :c].permute(0, 3, 1, 2) if with_res else a
            zt.backward(dz[..., :c].permute(0, 3, 1, 2))
            assert float((val['z'][..., :c] - zt.detach().permute(0, 2, 3, 1)).abs().max()) < 1e-12
            assert float(val['z'][..., c:].abs().max()) == 0.0
            assert float((val['dy'][..., :c] - x.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12
            assert float(val['dy'][..., c:].abs().max()) == 0.0
            assert float((val['chansum'] - cs0 - x.grad.sum(dim=(0, 2, 3))).abs().max()) < 1e-12
            if affine:
                assert float((val['dgamma'] - dg0 - gt.grad).abs().max()) < 1e-12 and float((val['dbeta'] - db0 - bt.grad).abs().max()) < 1e-12
            if running:
                assert float((val['running_mean'] - rm).abs().max()) < 1e-12 and float((val['running_var'] - rv).abs().max()) < 1e-12
            dims = (0, 2, 3) if scope == L.NORM_BATCH else (2, 3)
            xd = x.detach()
            assert float((val['mean'][:, :c] - xd.mean(dim=dims, keepdim=True).reshape(-1, c)).abs().max()) < 1e-12
            assert float((val['rstd'][:, :c] - (xd.var(dim=dims, unbiased=False, keepdim=True) + R.EPS).rsqrt().reshape(-1, c)).abs().max()) < 1e-12


def test_a_negative_momentum_leaves_the_running_statistics_untouched():
    y = torch.randn(2, 4, 4, 8, generator=torch.Generator().manual_seed(1))
    rm0, rv0 = torch.full((8,), 0.25), torch.full((8,), 1.5)
    val, bnd = R.reference(y, 8, L.NORM_BATCH, L.ACT_NONE, running=(rm0, rv0), momentum=-1.0)
    assert torch.equal(val['running_mean'], rm0.double()) and torch.equal(val['running_var'], rv0.double())
    assert float(bnd['running_mean'].max()) == 0.0 and float(bnd['running_var'].max()) == 0.0


def test_the_table_reaches_what_it_is_there_for():
    R.check_sweep_geometry()


# ------------------------------------------------------------------------------------------------ the emulation
def _round(v, dtype):
    return v if dtype == torch.float32 else torch.from_numpy(v).to(dtype).float().numpy()


def _serial(t, axis):
    """fp32 sum along `axis` in index order, starting from 0"""
    acc = np.zeros(t.shape[:axis] + t.shape[axis + 1:], dtype=f32)
    for i in range(t.shape[axis]):
        acc = acc + np.take(t, i, axis=axis)
    return acc


def _lanes(part, nacc):
    """part [K, ...]: lane kl of 32 takes K entries kl, kl + 32, ... into accumulator (position mod nacc); the accumulators are joined pairwise in fp32, the
    32 lanes in fp64"""
    K = part.shape[0]
    J = R.cdiv(K, 32)
    p = np.zeros((J * 32,) + part.shape[1:], dtype=f32)
    p[:K] = part
    p = p.reshape((J, 32) + part.shape[1:])
    acc = [np.zeros(p.shape[1:], dtype=f32) for _ in range(nacc)]
    for j in range(J):
        acc[j % nacc] = acc[j % nacc] + p[j]
    while len(acc) > 1:
        acc = [acc[i] + acc[i + 1] for i in range(0, len(acc), 2)]
    return acc[0].astype(np.float64).sum(axis=0)


class Emulation:
    """numpy fp32 arithmetic in the order csrc/norm.hip documents.  `mut` names one deliberate defect (MUTATIONS)."""

    def __init__(self, case, scope, dtype, t, mut=None):
        (self.N, self.H, self.W, self.Cp), self.C = case
        self.scope, self.dtype, self.mut = scope, dtype, mut
        self.HW = self.H * self.W
        self.ge = R.geometry(self.N, self.HW, self.Cp)
        rows = set(self.ge['col_rows'])
        assert len(rows) == 1, 'the emulation handles one rows value per tensor (true of every row of the sweep)'
        self.rows = rows.pop()
        self.y = t['y'].numpy().reshape(self.N, self.HW, self.Cp)
        pad = lambda v, fill: np.concatenate([np.full(self.C, fill, f32) if v is None else v.numpy().astype(f32), np.zeros(self.Cp - self.C, f32)])
        self.gamma, self.beta = pad(t['gamma'], 1.0), pad(t['beta'], 0.0)
        self.affine = t['gamma'] is not None
        self.real = np.arange(self.Cp) < self.C

    def live(self):
        """is the mutated path exercised by this geometry at all?"""
        ge, m = self.ge, self.mut
        if m == 'drop_thread_row':
            return ge['ppc'] >= self.rows
        if m == 'count_from_chunks':
            return ge['nchunks'] * ge['ppc'] != self.HW
        if m in ('batch_mean_at_instance_scope', 'c1_from_image_0'):
            return self.N > 1 and self.scope == L.NORM_INSTANCE
        if m == 'running_var_biased':
            return self.scope == L.NORM_BATCH
        return True

    # per-(image, channel) sums of two addend tensors [N, HW, Cp]: norm_partial_kernel + norm_chunk_sum_kernel
    def _sums(self, t1, t2):
        ge, rows = self.ge, self.rows
        nch, ppc = ge['nchunks'], ge['ppc']
        iters = R.cdiv(ppc, rows)
        out = []
        for t in (t1, t2):
            if self.mut == 'drop_last_pixel':
                t = t.copy()
                t[:, self.HW - 1] = 0
            p = np.zeros((self.N, nch * ppc, self.Cp), dtype=f32)
            p[:, :self.HW] = t
            p = p.reshape(self.N, nch, ppc, self.Cp)
            q = np.zeros((self.N, nch, iters * rows, self.Cp), dtype=f32)
            q[:, :, :ppc] = p
            per_thread = _serial(q.reshape(self.N, nch, iters, rows, self.Cp), 2)          # [N, nch, rows, Cp]
            if self.mut == 'drop_thread_row':
                per_thread[:, :, rows - 1] = 0
            part = _serial(per_thread, 2)                                                  # [N, nch, Cp]
            out.append(_lanes(np.moveaxis(part, 1, 0), 4))                                 # [N, Cp] float64
        return out

    def forward_stats(self, rm0=None, rv0=None, momentum=-1.0):
        N, Cp = self.N, self.Cp
        a1, a2 = self._sums(self.y, self.y * self.y)
        hw = self.ge['nchunks'] * self.ge['ppc'] if self.mut == 'count_from_chunks' else self.HW
        running = None
        if self.scope == L.NORM_INSTANCE:
            if self.affine:
                a1, a2 = a1.astype(f32).astype(np.float64), a2.astype(f32).astype(np.float64)
            cnt = float(hw)
            mu = a1 / cnt
            if self.mut == 'batch_mean_at_instance_scope':
                mu = np.broadcast_to(mu.mean(axis=0, keepdims=True), mu.shape)
            var = np.maximum(a2 / cnt - mu * mu, 0.0)
        else:
            s1, s2 = a1.astype(f32).astype(np.float64).sum(axis=0), a2.astype(f32).astype(np.float64).sum(axis=0)
            cnt = float(N * hw)
            mu = s1 / cnt
            var = np.maximum(s2 / cnt - mu * mu, 0.0)
            if rm0 is not None and momentum >= 0:
                m = f32(momentum)
                unb = var if self.mut == 'running_var_biased' else var * cnt / (cnt - 1.0)
                rm = (f32(1) - m) * rm0.numpy().astype(f32) + m * mu[:self.C].astype(f32)
                rv = (f32(1) - m) * rv0.numpy().astype(f32) + m * unb[:self.C].astype(f32)
                running = (rm, rv)
            mu, var = np.broadcast_to(mu, (N, Cp)), np.broadcast_to(var, (N, Cp))
        rs = (1.0 / np.sqrt(var + np.float64(f32(1e-5)))).astype(f32)
        if self.mut == 'stats_from_the_neighbour_channel':
            swap = np.arange(Cp) ^ 1
            mu, rs = mu[:, swap], rs[:, swap]
        sc = np.where(self.real, self.gamma * rs, f32(0)).astype(f32)
        sh = np.where(self.real, self.beta - mu.astype(f32) * sc, f32(0)).astype(f32)
        return np.stack([mu.astype(f32), rs, sc, sh]), running

    def apply(self, stats, act, res):
        sc, sh = stats[2][:, None, :], stats[3][:, None, :]
        nv = self.y * sc + sh
        r = None if res is None else res.numpy().reshape(self.y.shape)
        if self.mut == 'residual_before_the_activation' and r is not None:
            nv, r = nv + r, None
        v = nv if act == L.ACT_NONE else np.where(nv > 0, nv, f32(0) if act == L.ACT_RELU else f32(0.2) * nv)
        if r is not None:
            v = v + r
        return _round(v.astype(f32), self.dtype).reshape(self.N, self.H, self.W, self.Cp)

    def backward(self, stats, act, dz, dg0, db0, cs0):
        N, HW, Cp, C = self.N, self.HW, self.Cp, self.C
        mu, rs, sc, sh = (stats[i][:, None, :] for i in range(4))
        d = dz.numpy().reshape(N, HW, Cp)
        nv = self.y * sc + sh
        pos = (self.y if self.mut == 'mask_from_y' else nv) > 0
        dn = d if act == L.ACT_NONE else np.where(pos, d, f32(0) if act == L.ACT_RELU else f32(0.2) * d).astype(f32)
        s1, s2 = self._sums(dn, dn * (self.y - mu) * rs)
        s1, s2 = s1.astype(f32).astype(np.float64), s2.astype(f32).astype(np.float64)
        if self.scope == L.NORM_INSTANCE:
            c1, c2 = (s1 / HW).astype(f32), (s2 / HW).astype(f32)
            if self.mut == 'c1_from_image_0':
                c1 = np.broadcast_to(c1[:1], c1.shape)
        else:
            m = float(N * HW)
            c1, c2 = np.broadcast_to((s1.sum(axis=0) / m).astype(f32), (N, Cp)), np.broadcast_to((s2.sum(axis=0) / m).astype(f32), (N, Cp))
        out = {'c1': c1, 'c2': c2}
        if dg0 is not None:
            keep = f32(0) if self.mut == 'overwrite_not_accumulate' else f32(1)
            out['dgamma'] = keep * dg0.numpy().astype(f32) + s2.sum(axis=0)[:C].astype(f32)
            out['dbeta'] = keep * db0.numpy().astype(f32) + s1.sum(axis=0)[:C].astype(f32)
        mr = -stats[0] * stats[1]
        gr = np.where(self.real, self.gamma * stats[1], f32(0)).astype(f32)
        xh = self.y * rs + mr[:, None, :]
        k2 = f32(0) if self.mut == 'no_c2_term' else c2[:, None, :]
        o = (gr[:, None, :] * ((dn - c1[:, None, :]) - xh * k2)).astype(f32)
        # channel sums: thread (block b, row r) adds pixels b rows + r + j blocks rows, j = 0, 1, ...; rows joined serially; then the lanes of norm_bias_final_kernel
        bx, rows = self.ge['blocks'], self.rows
        J = R.cdiv(HW, bx * rows)
        q = np.zeros((N, J * bx * rows, Cp), dtype=f32)
        q[:, :HW] = o
        bpart = _serial(_serial(q.reshape(N, J, bx, rows, Cp), 1), 2)          # [N, bx, Cp]
        tot = _lanes(bpart.reshape(N * bx, Cp), 8)[:C].astype(f32)
        out['chansum'] = (f32(0) if self.mut == 'overwrite_not_accumulate' else f32(1)) * cs0.numpy().astype(f32) + tot
        out['dy'] = _round(o, self.dtype).reshape(N, self.H, self.W, Cp)
        return out


MUTATIONS = ['drop_last_pixel', 'drop_thread_row', 'count_from_chunks', 'stats_from_the_neighbour_channel', 'batch_mean_at_instance_scope', 'running_var_biased',
             'mask_from_y', 'residual_before_the_activation', 'no_c2_term', 'c1_from_image_0', 'overwrite_not_accumulate']
FORWARD_MUTATIONS = set(MUTATIONS[:6]) | {'residual_before_the_activation'}
MOMENTUM = 0.1


@functools.lru_cache(maxsize=2)
def _setup(case, scope, dtype):
    """inputs, Reference and the preloaded accumulators of one (case, scope, dtype); dgamma / dbeta also at instance scope when it has no affine of its own:
    the kernel then returns the plain sums"""
    t = R.make_inputs(case, scope, dtype)
    c = case[1]
    ref = R.Reference(t['y'], c, scope, t['gamma'], t['beta'])
    gen = torch.Generator().manual_seed(6)
    pre = {k: torch.randn(c, generator=gen) for k in ('dgamma', 'dbeta', 'chansum')}
    pre['rm'], pre['rv'] = 0.1 * torch.randn(c, generator=gen), 1 + 0.1 * torch.rand(c, generator=gen)
    return t, ref, pre


def _judge(case, scope, dtype, act, with_res, mut=None, forward=True, backward=True):
    """worst err / bound over every output of the emulation; {} of ratios per output"""
    t, ref, pre = _setup(case, scope, dtype)
    c = case[1]
    emu = Emulation(case, scope, dtype, t, mut)
    if mut is not None and not emu.live():
        return None
    ratios, reports = {}, []

    def cmp(key, got, want, bnd, ge=None):
        ratios[key], rep = R.compare(torch.from_numpy(np.array(got)), want, bnd, ge)
        if rep:
            reports.append(f'{key}: {rep}')
    batch = scope == L.NORM_BATCH
    if forward:
        stats, running = emu.forward_stats(pre['rm'], pre['rv'], MOMENTUM if batch else -1.0)
        sb = ref.stat_bounds()
        for i, k in enumerate(('mean', 'rstd', 'scale', 'shift')):
            cmp(k, stats[i], ref.stats()[k], sb[k])
        if batch:
            (rm, rv), (b_rm, b_rv) = ref.running(pre['rm'], pre['rv'], MOMENTUM)
            cmp('running_mean', running[0], rm, b_rm)
            cmp('running_var', running[1], rv, b_rv)
        res = t['res'] if with_res else None
        z, b_z = ref.forward(act, res, dtype)
        cmp('z', emu.apply(stats, act, res), z, b_z, ref.ge)
    if backward:
        val, bnd = ref.backward(act, t['dz'], dtype, pre['dgamma'], pre['dbeta'], pre['chansum'])
        got = emu.backward(ref.stats32.numpy(), act, t['dz'], pre['dgamma'], pre['dbeta'], pre['chansum'])
        for k in ('c1', 'c2', 'dgamma', 'dbeta', 'chansum', 'dy'):
            cmp(k, got[k], val[k], bnd[k], ref.ge if k == 'dy' else None)
    return ratios, '\n'.join(reports)


@pytest.mark.parametrize('scope', SCOPES, ids=SCOPE_NAME.get)
@pytest.mark.parametrize('case', R.SWEEP, ids=R.case_id)
def test_the_bound_holds_for_the_documented_summation_order(case, scope):
    """and every case of the sweep converges under the kink repair"""
    big = np.prod(case[0]) > 2 ** 21
    for dtype in (torch.float32,) if big else (torch.float32, torch.bfloat16):
        t, _, _ = _setup(case, scope, dtype)
        assert t['near_kink'] == 0, 'the kink repair did not converge'
        for act, with_res in ((L.ACT_RELU, True),) if big else ((L.ACT_RELU, True), (L.ACT_LRELU, False), (L.ACT_NONE, True)):
            ratios, report = _judge(case, scope, dtype, act, with_res)
            worst = max(ratios, key=ratios.get)
            print(f'{R.case_id(case)} {SCOPE_NAME[scope]} {dtype} act {act}: worst err/bound {ratios[worst]:.3f} ({worst}); ' +
                  ' '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
            assert ratios[worst] <= 1.0 and not report, report


@pytest.mark.parametrize('mutation', MUTATIONS)
@pytest.mark.parametrize('case', R.SWEEP, ids=R.case_id)
def test_the_bound_rejects_a_subtly_wrong_kernel(case, mutation):
    live = 0
    for scope in SCOPES:
        fwd = mutation in FORWARD_MUTATIONS
        out = _judge(case, scope, torch.float32, L.ACT_RELU, True, mutation, forward=fwd, backward=not fwd)
        if out is None:
            continue
        live += 1
        ratios, report = out
        worst = max(ratios, key=ratios.get)
        print(f'{R.case_id(case)} {SCOPE_NAME[scope]} {mutation}: worst err/bound {ratios[worst]:.3g} ({worst})')
        assert ratios[worst] > 1.0 and report, f'{mutation} passed the comparer at {SCOPE_NAME[scope]} scope: {ratios}'
    if not live:          # nothing to reject: one image (the two per-image mutations), no thread row without a pixel, or chunks that tile the map exactly
        (n, h, w, cp), _ = case
        ge = R.geometry(n, h * w, cp)
        assert {'drop_thread_row': ge['ppc'] < ge['col_rows'][0], 'count_from_chunks': ge['nchunks'] * ge['ppc'] == h * w,
                'batch_mean_at_instance_scope': n == 1, 'c1_from_image_0': n == 1}[mutation]


def test_the_comparer_says_where():
    case = R.SWEEP[4]          # Cp = 24, rows = 85, chunks of 63 pixels
    out = _judge(case, L.NORM_INSTANCE, torch.float32, L.ACT_RELU, True, 'drop_last_pixel', backward=False)
    assert 'by pixel mod rows' in out[1] and 'by chunk index' in out[1] and 'by channel mod 8' in out[1] and 'by 8-channel column' in out[1] and 'by image' in out[1]
    t, ref, _ = _setup(case, L.NORM_INSTANCE, torch.float32)
    z, b = ref.forward(L.ACT_NONE, None, torch.float32)
    got = z.clone()
    ppc = ref.ge['ppc']
    for p in (ppc - 1, 2 * ppc - 1, 3 * ppc):          # two last pixels of a chunk and one first, image 1, channel 10
        got[1, p // 36, p % 36, 10] += 1.0
    got[2, 0, 5, 3] = float('nan')
    worst, report = R.compare(got, z, b, ref.ge)
    assert worst == float('inf') and '4 of ' in report
    assert 'first pixel of a chunk: 1, last pixel of a chunk: 2' in report and 'by 8-channel column {1: 3, 0: 1}' in report, report
    assert 'by channel mod 8    {2: 3, 3: 1}' in report and 'by image            {1: 3, 2: 1}' in report, report


# ------------------------------------------------------------------------------------------------ the workspace contract
def _desc(n, h, w, cp):
    d = L.NormDesc()
    d.N, d.H, d.W, d.Cp, d.C = n, h, w, cp, cp
    d.y_pstride = d.z_pstride = d.r_pstride = cp
    d.dtype, d.scope, d.act, d.eps, d.momentum, d.ext_nchunks = L.DL_BF16, L.NORM_INSTANCE, L.ACT_NONE, 1e-5, -1.0, 0
    return d


@pytest.mark.parametrize('n', list(range(1, 18)) + [31, 64, 1024, 2049])
def test_the_workspace_covers_every_row_the_kernels_write(n):
    """dl_norm_ws_floats against a restatement of what the launches index: N nchunks 2 Cp partials, 4 N Cp per-image values, and one row of Cp bias partials
    per block of the apply grid (norm_bwd_apply_kernel writes row n gridDim.x + blockIdx.x).  The (H W, Cp) pairs reach the cap of the grid: 16 rows pixels
    per block, and each map has at least 2048 of them (only the descriptor is that large: nothing is allocated), at the narrowest, a 24-channel and the
    widest tensor; the single pixel is the other end."""
    lib = L.load()
    for h, w, cp in ((1024, 1024, 128), (4096, 4096, 8), (2048, 2048, 24), (256, 256, 2048), (1, 1, 8)):
        ge = R.geometry(n, h * w, cp)
        assert ge['blocks'] * n <= max(R.BIAS_PART_ROWS, n)
        if h * w > 1:
            assert R.cdiv(h * w, ge['col_rows'][0] * 16) >= 2048 and ge['blocks'] == max(1, R.BIAS_PART_ROWS // n), 'this pair does not reach the cap'
        got = int(lib.dl_norm_ws_floats(C.byref(_desc(n, h, w, cp))))
        need = R.ws_floats(n, h * w, cp)
        assert got >= need, f'N={n} {h}x{w} Cp={cp}: {got} floats reserved, {need} indexed ({ge["blocks"]} x {n} apply blocks)'
        # the same with a producer's chunk count in place of the norm's own (dl_conv_forward's fused statistics)
        d = _desc(n, h, w, cp)
        d.ext_nchunks = 3 * ge['nchunks']
        assert int(lib.dl_norm_ws_floats(C.byref(d))) >= R.ws_floats(n, h * w, cp, d.ext_nchunks)


def test_a_cap_rounded_up_overflows_the_region():
    """the rule this contract replaced: ceil(2048 / N) blocks per image are more than 2048 rows at every N that does not divide 2048"""
    assert [n * R.cdiv(2048, n) for n in (3, 5, 6, 7, 9)] == [2049, 2050, 2052, 2051, 2052]
    assert all(n * max(1, R.BIAS_PART_ROWS // n) <= max(R.BIAS_PART_ROWS, n) for n in range(1, 4100))
