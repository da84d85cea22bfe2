"""CPU checks of the weight-gradient test infrastructure (tests/wgrad_ref.py, tests/wgrad_cases.py): no GPU, no kernel.

1. descriptor_of() + reference() equals a second, independent float64 evaluation on every row to 1e-12: an einsum over explicitly gathered taps of the P / Q problem
   that descriptor_of() describes.  The reference itself is autograd through the LAYER, so the two can only agree if the roles, the step, the padding and the
   gradient layout of the descriptor are the layer's.
2. emulate() without a mutation is inside bound() on every row, policy and split-K of the table, with and without `accumulate`.
3. every mutation of wgrad_ref.MUTATIONS is OUT of bound on every launch where wgrad_ref.live() says its path is live -- the bound is sharp enough at the table's
   sizes to reject the faults tests/test_gpu_wgrad.py exists for.  Live launches per mutation:
       drop_last_pixel, accumulate_ignores_g0   every launch
       drop_range_last_pixel, skip_last_slab    split-K >= 2 with a non-empty second / last range
       empty_slab_junk                          the split-K 3 launches of the K = 120 rows (ranges of 64, 56 and 0 pixels)
       pad_reads_col0                           zero padding >= 1 (not the stacked head: its horizontal taps are shift_stack's)
       last_row_step1                           stride 2 with more than one P row
       act_not_rerounded                        LeakyReLU under bf16 / f32b, ReLU under f32b (ReLU of a bf16 value is a bf16 value)
       strict_*                                 the strict launches (strict_q_lo_first_step_only: those with a range longer than one K step)
       pad_column_onto_last                     CB < CBp
       stack_swaps_kh_kw                        the stacked head
       ca_tail_from_tile0                       the CAp = 136 row
   Smallest rejecting ratio (worst err / bound over the gradient, minimum over the live launches; test_every_mutation_is_rejected prints them and asserts > 1):
       drop_last_pixel 1.2e3 (c4-head-2x8x64/strict)      drop_range_last_pixel 360 (w4-3x3x128/sk2)          empty_slab_junk 990 (gen-ca16/strict/sk3)
       skip_last_slab 7.1e3 (w4-3x3x128/sk2)              accumulate_ignores_g0 52 (c4-stem-2x8x64/strict)    pad_reads_col0 1.6e3 (c4-head-2x8x64/strict)
       last_row_step1 2.3e4 (gen-k4s2-6to64/strict)       act_not_rerounded 166 (gen-k4s2-6to64/bf16)         strict_drop_hi_lo 3.9 (c4-stem-2x8x64)
       strict_q_lo_first_step_only 3.9 (c4-stem-2x8x64)   strict_last_pixel_lo_zero 4.9 (c4-head-2x8x64)      pad_column_onto_last 1.8e3 (c4-stem-2x8x64/strict)
       stack_swaps_kh_kw 6.3e4 (gen-head-stack/strict)    ca_tail_from_tile0 2.7e4 (gen-ca136/strict)
   The three strict faults are closest to the bound on the K = 1024 rows of the persistent c4 kernel (the summation term grows with K^2 against one product); on
   the K <= 120 rows of the generic and the direct-to-LDS kernels they stand at 14 x and more.
4. the kernel name of every launch through dl_wgrad_plan (answers on the host) when the library is built."""
import pytest
import torch

import wgrad_cases as WC
import wgrad_ref as WR
from deepliif_amd import _lib as L
from deepliif_amd._lib import WGRAD_C4_PARTS

_CACHE = {}


def _case(row, policy):
    """(inputs, (ref, S, K)) of a (row, policy): computed once, never modified"""
    key = (row.id, policy)
    if key not in _CACHE:
        data = WR.inputs(row, policy)
        _CACHE[key] = (data, WR.reference(row, data[0], data[1], policy))
    return _CACHE[key]


def _second_evaluation(row, policy, x, dy):
    """float64 einsum over explicitly gathered taps of the (P, Q, step, pad, pad_mode) problem of descriptor_of()"""
    d = WR.descriptor_of(row)
    t = {'x': (x, row.in_act, row.cin), 'dy': (dy, L.ACT_NONE, row.cout)}
    (P, pa, pc), (Q, qa, qc) = t[d.p_role], t[d.q_role]
    assert (pa, qa) == (d.p_act, d.q_act) and (pc, qc) == (d.CA, d.CB)
    Pv, Qv = WR.model_values(P, pa, policy)[..., :pc], WR.model_values(Q, qa, policy)[..., :qc]
    N, Hp, Wp, _ = Pv.shape
    Hq, Wq = Qv.shape[1:3]
    out = torch.zeros(d.gshape, dtype=torch.float64)
    for kh in range(d.k):
        for kw in range(d.k):
            hi, wi = torch.arange(Hp) * d.step + kh - d.pad, torch.arange(Wp) * d.step + kw - d.pad
            if d.pad_mode == L.PAD_ZERO:
                m = ((hi >= 0) & (hi < Hq))[:, None] & ((wi >= 0) & (wi < Wq))[None, :]
                g = Qv[:, hi.clamp(0, Hq - 1)][:, :, wi.clamp(0, Wq - 1)] * m.double()[None, :, :, None]
            else:
                g = Qv[:, WR._border(d.pad_mode, hi, Hq)][:, :, WR._border(d.pad_mode, wi, Wq)]
            out[:, :, kh, kw] = torch.einsum('nhwa,nhwb->ab', Pv, g)
    return out


@pytest.mark.parametrize('row', WC.ROWS, ids=lambda r: r.id)
def test_reference_equals_an_independent_evaluation(row):
    for policy in row.policies:
        (x, dy, _), (ref, S, K) = _case(row, policy)
        second = _second_evaluation(row, policy, x, dy)
        assert ref.shape == second.shape
        scale = float(S.max())
        assert float((ref - second).abs().max()) <= 1e-12 * scale, (policy, float((ref - second).abs().max()), scale)
        assert float(S.min()) >= 0 and float(K.min()) >= 0 and float(K.max()) <= row.n * max(row.H * row.W, dy.shape[1] * dy.shape[2])


def test_inputs_follow_the_policy():
    row = WC.ROWS[0]
    x, dy, _ = WR.inputs(row, 'bf16')
    assert torch.equal(x, x.bfloat16().float()) and torch.equal(dy, dy.bfloat16().float())
    x3, dy3, _ = WR.inputs(row, 'strict')
    assert not torch.equal(x3, x3.bfloat16().float())          # full mantissas: the lo planes are not zero
    assert torch.equal(WR.inputs(row, 'strict')[0], x3)       # fixed seed
    for r in WC.ROWS:
        xr, dyr, g0 = WR.inputs(r, r.policies[0])
        shapes = WR._shapes(r)
        assert tuple(xr.shape) == shapes[0] and tuple(WR.operands(r, xr, dyr)[0 if WR.descriptor_of(r).p_role == 'dy' else 1].shape) == shapes[1], r.id
        assert tuple(g0.shape) == shapes[2]
        assert float(xr[..., r.cin:].abs().sum()) == 0.0 and float(dyr[..., r.cout:].abs().sum()) == 0.0, r.id          # padding channels
        if r.cin >= 32:
            assert float(xr[:, 0, 0, :r.cin].abs().mean()) > 4 and float(xr[:, -1, -1, :r.cin].abs().mean()) > 4, r.id   # the planted edge pixels (E|8 z| = 6.4)


def _ratio(row, policy, splitk, accumulate, mutation=None):
    data, (ref, S, K) = _case(row, policy)
    g0 = data[2] if accumulate else None
    got = WR.emulate(row, policy, splitk, accumulate, mutation, data)
    want = ref if g0 is None else ref + g0.double()
    return WR.compare(got, want, WR.bound(ref, S, K, policy, g0), WR.descriptor_of(row))


@pytest.mark.parametrize('launch', WC.ALL_LAUNCHES, ids=WC.launch_id)
def test_emulation_is_in_bound(launch):
    row, policy, splitk = launch
    for accumulate in (False, True):
        worst, report = _ratio(row, policy, splitk, accumulate)
        assert worst <= 1.0 and not report, f'accumulate={accumulate}\n{report}'


def _effective(row, policy, splitk):
    (x, dy, _), _ = _case(row, policy)
    P, Q = WR.operands(row, x, dy)
    return WR.effective_splitk(row, policy, splitk, P, Q)


@pytest.mark.parametrize('mutation', WR.MUTATIONS)
def test_every_mutation_is_rejected(mutation):
    smallest, where, n_live = float('inf'), None, 0
    for row, policy, splitk in WC.ALL_LAUNCHES:
        if not WR.live(mutation, row, policy, _effective(row, policy, splitk)):
            continue
        n_live += 1
        worst, report = _ratio(row, policy, splitk, True, mutation)
        assert worst > 1.0 and report, f'{mutation} survives on {WC.launch_id((row, policy, splitk))}: worst err/bound {worst:.4g}'
        if worst < smallest:
            smallest, where = worst, WC.launch_id((row, policy, splitk))
    assert n_live > 0, f'{mutation}: no live launch in the table'
    print(f'{mutation}: {n_live} live launches, smallest err/bound {smallest:.3g} at {where}')


def test_a_mutation_is_a_no_op_where_it_is_not_live():
    """live() is the condition, not a convenience: where it says False the mutated emulation gives the same bits"""
    for mutation in WR.MUTATIONS:
        if mutation == 'accumulate_ignores_g0':
            continue
        for row, policy, splitk in WC.ALL_LAUNCHES[::7]:
            if WR.live(mutation, row, policy, _effective(row, policy, splitk)):
                continue
            data, _ = _case(row, policy)
            assert torch.equal(WR.emulate(row, policy, splitk, True, mutation, data), WR.emulate(row, policy, splitk, True, None, data)), (mutation, row.id)


def plan_splitk(row, splitk):
    return WGRAD_C4_PARTS if row.form == 'c4' else (splitk or 1)


def test_routing_of_every_launch():
    try:
        lib = L.load('bf16')
    except L.HipLibraryError as e:
        pytest.skip(f'library not built: {e}')
    for row, policy, splitk in WC.ALL_LAUNCHES:
        xs, dys, _ = WR._shapes(row)
        d = WR.descriptor_of(row)
        ps, qs = (dys, xs) if d.p_role == 'dy' else (xs, dys)
        rc, _, _, name = WR.plan(lib, WR.wgrad_desc(row, policy, plan_splitk(row, _effective(row, policy, splitk)), ps, qs))
        assert rc >= 0 and name == row.kernel, (WC.launch_id((row, policy, splitk)), name)
        if 'multi' in row.extras:
            assert rc == 1, row.id
