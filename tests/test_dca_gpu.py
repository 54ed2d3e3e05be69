"""GPU: Deep Covariance Alignment (rgda_dca_context, rgda_dca_loss) -- the op against float64, against a CPU emulation of
the stated contract and against the reference goldens; the modules of regda_amd.dca_modules through autograd;
AlignStep(dca_weight=) against the CPU stage-2 step composed with the restated term (tests/dca_ref.py).

Shapes (dca_ref.CASES), the smallest at which the kernels can still go wrong:
    b2_k6_c32_5x7      one ragged pixel tile, the narrowest channel count (half a channel tile)
    b4_k7_c96_9x9      hw = 81 just past 64: two gradient pixel tiles, the second ragged; a ragged 64-channel tile
    b2_k16_c64_8x8     the most classes: every row of the MFMA's class operand in use
    b2_k6_c64_33x33    1089 pixels: past the production 1024, nine 128-pixel context tiles, the last ragged
    b4_k6_c2048_16x16  the production width: 32 channel tiles, 8 gradient channel tiles, two full context tiles

Bounds.  Loose (kernel against float64): tests/golden/dca_tolerances.json, per case and kind 3 x the deviation of the
emulated contract from float64 that tests/golden/derive_dca_tolerances.py observes.  Against the reference's golden
values the reference's own fp32 noise comes on top (triangle inequality), taken as tests/test_dca_cpu.py derives it.

Per element (rgda_dca_context against float64).  S[b,k,c] is a sum of hw fp32 products; every addition rounds by at
most 2^-24 of a partial sum that is at most T Z = sum_p |x| P, with independent signs sqrt(hw) 2^-24 T Z; P itself
carries the roundings of exp, the class sum and the division (a few 2^-24 each, independent from pixel to pixel), Z the
same, the division one more: one standard deviation of v is (sqrt(hw) + 8) 2^-24 T with T = sum_p |x| P / Z, and the test
allows four.  The normalisation over the classes gives du_k = (dv_k - u_k sum_k' u_k' dv_k') / N, at most twice the
largest dv of that (image, channel) over N: |du| <= 8 (sqrt(hw) + 8) 2^-24 max_k T / N.  Z: 4 (sqrt(hw) + 8) 2^-24 Z.

Tight (kernel against dca_emulated: the same precision, another order of the sums).  The emulation adds the pixels one
after the other in fp32 -- chains of hw additions where a wavefront of the kernel adds four pixels per MFMA step in
chains of hw / 16 steps, then a tree over the four wavefronts, so the emulation's rounding noise is the larger --
ascending or descending (and the channel sums flipped).  The deviation e_order between
these two orders of the emulation is what one change of summation order costs on that case's inputs; two independent
orders differ by sqrt(2) of one order's noise, and so do the kernel and the emulation.  The test allows 4 e_order, plus a
floor for what is no summation order (the device's hardware exp2, reciprocal and sqrt against the host's library ones:
exp((l - max)) through exp2 carries up to (|l - max| + 2) 2^-24, which is a few roundings on the entries near the maximum
that carry a pixel's weight and at most 14 at |l - max| = 12, where the entry weighs e^-12 of its pixel: 16 roundings of
2^-24 in all):
    u        relative norm  4 e_order(u) + 16 2^-24
    loss     relative       4 e_order(L) + (sqrt(c) + 16) 2^-24 K / |L|: every entry of R is a quotient of three channel
             sums whose partial sums are bounded by the product of the two norms, so dR <= (sqrt(c) + 16) 2^-24 and
             dL <= that times K = sum_ij |dL/dR_ij| (cov); mse is a sum of squares, K = L.
    rows     both sides store bf16: with e_g = 4 e_order(fp32 rows) + 16 2^-24 the fp32 values differ by e_g (relative
             norm); a bf16 rounding flips with probability e_g / 2^-8 and then moves the element by at most 2^-7 of it:
             relative norm sqrt(e_g / 2^-8) 2^-7 + e_g."""
import json
import os

import numpy as np
import pytest
import torch

from dca_ref import (CASES, case_inputs, check_cov_conditions, cov_conditions, dca_emulated, dca_restated, golden_cases,
                     make_inputs, probs, random_inputs, relnorm)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = json.load(open(os.path.join(HERE, 'golden', 'dca_tolerances.json')))
U = 2.0 ** -24
_CACHE = {}


def reference(key, sides, pred_kind='logits2', kind='cov', ignore_bg=True):
    """float64, the emulation and the emulation in its second order, computed once per key and shared"""
    key = (key, pred_kind, kind, ignore_bg)
    if key not in _CACHE:
        _CACHE[key] = (dca_restated(sides, pred_kind, kind, ignore_bg), dca_emulated(sides, pred_kind, kind, ignore_bg),
                       dca_emulated(sides, pred_kind, kind, ignore_bg, reverse=True))
    return _CACHE[key]


def cuda_side(side):
    f, preds = side
    return f.cuda(), tuple(p.cuda() for p in preds)


def run(sides, pred_kind='logits2', kind='cov', ignore_bg=True, weight=1.0, want=(True, True), bufs=None, accumulate=False,
        loss=None):
    """-> (loss float, rows_a, rows_b: bf16 on the CPU or None)"""
    from regda_amd import ops
    (fa, pa), (fb, pb) = [s if s[0].is_cuda else cuda_side(s) for s in sides]
    if bufs is None:
        bufs = [torch.empty(f.shape[0] * f.shape[2] * f.shape[3], f.shape[1], dtype=BF, device='cuda') if w else None
                for f, w in zip((fa, fb), want)]
    out = ops.dca_loss(fa, pa, fb, pb, pred_kind, kind, ignore_bg, weight, loss=loss, dfeat_a=bufs[0], dfeat_b=bufs[1],
                       accumulate=accumulate)
    return out.item(), *(None if b is None else b.cpu() for b in bufs)


def tight_bounds(e, e2, c, kind):
    eu = max(relnorm(e2['u_a'], e['u_a']), relnorm(e2['u_b'], e['u_b']))
    el = abs(e2['loss'] - e['loss']) / abs(e['loss'])
    K = float(e['W'].abs().sum()) if kind == 'cov' else abs(e['loss'])
    eg = 4 * max(relnorm(e2['rows_a'], e['rows_a']), relnorm(e2['rows_b'], e['rows_b'])) + 16 * U
    return dict(u=4 * eu + 16 * U, loss=4 * el + (np.sqrt(c) + 16) * U * K / abs(e['loss']),
                rows=np.sqrt(eg / 2.0 ** -8) * 2.0 ** -7 + eg)


def check(tag, got, r, e, e2, c, kind, sides_with_grad='ab', loose=None):
    """loss and rows against the emulation (tight) and, with `loose` (the bounds of dca_tolerances.json), float64"""
    loss, rows = got[0], dict(a=got[1], b=got[2])
    tb = tight_bounds(e, e2, c, kind)
    t_l = abs(loss - e['loss']) / abs(e['loss'])
    print(tag, kind, 'loss', loss, 'emulated', e['loss'], 'rel', t_l, 'bound', tb['loss'], 'float64', r['loss'],
          'rel', abs(loss - r['loss']) / abs(r['loss']), 'bound', loose and loose['loss_rel'])
    assert t_l <= tb['loss'], (tag, kind, t_l, tb['loss'])
    for s in sides_with_grad:
        t_g = relnorm(rows[s], e['grad_' + s])
        l_g = relnorm(rows[s], r['rows_' + s])
        print(tag, kind, 'rows', s, 'against the emulation', t_g, 'bound', tb['rows'], 'against float64', l_g, 'bound',
              loose and loose['grad_rel'])
        assert t_g <= tb['rows'], (tag, kind, s, t_g, tb['rows'])
        if loose:
            assert l_g <= loose['grad_rel'], (tag, kind, s, l_g)
    if loose:
        assert abs(loss - r['loss']) / abs(r['loss']) <= loose['loss_rel'], (tag, kind)


@pytest.mark.parametrize('name', list(CASES))
def test_dca_context_per_element_against_float64(name):
    from regda_amd import ops
    sides = case_inputs(name)
    r, e, e2 = reference(name, sides)
    hw = CASES[name][3] * CASES[name][4]
    sd = np.sqrt(hw) + 8
    worst = 0.0
    for s, side in zip('ab', sides):
        f, preds = cuda_side(side)
        u, v, Z = (t.cpu().double() for t in ops.dca_context(f, preds, 'logits2', True, return_all=True))
        assert torch.equal(ops.dca_context(f, preds, 'logits2', True).cpu().double(), u)
        T, N = r['T_' + s][:, 1:], r['v_' + s].pow(2).sum(1, keepdim=True).sqrt()
        bz = 4 * sd * U * r['Z_' + s]
        bv = 4 * sd * U * T
        bu = 8 * sd * U * T.max(1, keepdim=True).values / N
        for what, got, ref, bound in (('Z', Z, r['Z_' + s], bz), ('v', v, r['v_' + s], bv), ('u', u, r['u_' + s], bu.expand_as(u))):
            ratio = ((got - ref).abs() / bound).max().item()
            print(name, s, what, 'largest deviation in units of its bound', ratio)
            assert ratio <= 1.0, (name, s, what, ratio)
        worst = max(worst, relnorm(u, r['u_' + s]))
        assert relnorm(u, e['u_' + s]) <= tight_bounds(e, e2, CASES[name][2], 'cov')['u'], (name, s)
    print(name, 'u relative norm against float64', worst, 'bound', TOL['bounds'][name]['cov']['u_rel'])
    assert worst <= TOL['bounds'][name]['cov']['u_rel']


@pytest.mark.parametrize('kind', ['cov', 'mse'])
@pytest.mark.parametrize('name', list(CASES))
def test_dca_loss_shapes(name, kind):
    """both sides receive a gradient (the ICR / MSE_intra form)"""
    sides = case_inputs(name)
    r, e, e2 = reference(name, sides, kind=kind)
    if kind == 'cov':
        check_cov_conditions(r['R'], name)
    check(name, run(sides, kind=kind), r, e, e2, CASES[name][2], kind, loose=TOL['bounds'][name][kind])


def test_dca_loss_matches_the_reference_goldens(gold):
    """CCR (target rows only), ICR (both halves) and MSE_cross minted from the reference's own module: the loose bounds
    plus the reference's own fp32 noise (fp32 restated against float64, margin 3, as in tests/test_dca_cpu.py)"""
    for name, g in golden_cases(gold('dca.npz')):
        sides = tuple((torch.from_numpy(g['feat_' + s]), (torch.from_numpy(g['l1_' + s]), torch.from_numpy(g['l2_' + s])))
                      for s in 'ab')
        for key, kind, want in (('ccr', 'cov', (False, True)), ('icr', 'cov', (True, True)), ('msecross', 'mse', (False, True))):
            if key + '_loss' not in g:
                continue
            r = dca_restated(sides, 'logits2', kind, True)
            f = dca_restated(sides, 'logits2', kind, True, dtype=torch.float32)
            loose = TOL['bounds'][name][kind]
            noise_l = 3 * max(abs(f['loss'] - r['loss']) / abs(r['loss']), 2.0 ** -23)
            loss, ra, rb = run(sides, kind=kind, want=want)
            lrel = abs(loss - float(g[key + '_loss'])) / abs(float(g[key + '_loss']))
            print(name, key, 'loss', loss, float(g[key + '_loss']), 'rel', lrel, 'bound', loose['loss_rel'] + noise_l)
            assert lrel <= loose['loss_rel'] + noise_l, (name, key, lrel)
            for s, rows in (('a', ra), ('b', rb)):
                if rows is None:
                    assert key + '_rows_' + s not in g
                    continue
                noise_g = 3 * max(relnorm(f['rows_' + s], r['rows_' + s]), 2.0 ** -23)
                grel = relnorm(rows, g[key + '_rows_' + s])
                print(name, key, 'rows', s, 'rel', grel, 'bound', loose['grad_rel'] + noise_g)
                assert grel <= loose['grad_rel'] + noise_g, (name, key, s, grel)


@pytest.mark.parametrize('pred_kind', ['prob', 'logits', 'logits2'])
@pytest.mark.parametrize('ignore_bg', [True, False])
def test_ignore_bg_and_every_pred_kind(pred_kind, ignore_bg):
    """on b4_k7_c96_9x9; 'prob' takes the fp32 softmax of the first logit map as given probabilities.  Against the
    emulation (tight) and float64, whose bound is the emulation's own deviation from float64 on these settings with the
    margin of 3 (as derive_dca_tolerances.py takes it for the default settings)"""
    name = 'b4_k7_c96_9x9'
    sides = case_inputs(name)
    if pred_kind == 'prob':
        sides = tuple((f, (p[0].softmax(1),)) for f, p in sides)
    elif pred_kind == 'logits':
        sides = tuple((f, (p[0],)) for f, p in sides)
    for kind in ('cov', 'mse'):
        r, e, e2 = reference(name, sides, pred_kind, kind, ignore_bg)
        if kind == 'cov':
            check_cov_conditions(r['R'], (name, pred_kind, ignore_bg))
        loose = dict(loss_rel=3 * max(abs(x['loss'] - r['loss']) / abs(r['loss']) for x in (e, e2)) + 3 * 2.0 ** -23,
                     grad_rel=3 * max(relnorm(torch.cat([x['grad_a'], x['grad_b']]), torch.cat([r['rows_a'], r['rows_b']]))
                                      for x in (e, e2)))
        got = run(sides, pred_kind, kind, ignore_bg)
        check((name, pred_kind, ignore_bg), got, r, e, e2, 96, kind, loose=loose)
        assert e['u_a'].shape[1] == (6 if ignore_bg else 7)


def test_unequal_image_counts_ccr_icr_and_mse_refused():
    """CCR with 2 source and 3 target images; ICR on a batch of 3 (halves of 1 and 2 images); mse with unequal counts is
    refused"""
    sides = make_inputs(2, 6, 64, 6, 7, 1.0, 3.0, 51, b_b=3)
    r, e, e2 = reference('b2_b3', sides)
    check_cov_conditions(r['R'], 'b2_b3')
    got = run(sides, want=(False, True))
    assert got[1] is None
    check('ccr 2+3', got, r, e, e2, 64, 'cov', 'b')
    (fa, pa), (fb, pb) = sides
    icr = ((fb[:1], tuple(p[:1] for p in pb)), (fb[1:], tuple(p[1:] for p in pb)))
    r, e, e2 = reference('b1_b2', icr)
    check_cov_conditions(r['R'], 'b1_b2')
    check('icr 1+2', run(icr), r, e, e2, 64, 'cov')
    with pytest.raises(ValueError):
        run(sides, kind='mse')


def test_accumulate_leaves_the_source_rows_and_adds_onto_the_target_rows():
    """one buffer for both domains, pre-filled: CCR with accumulate writes the target rows only -- the source rows keep
    their prior bit for bit -- and the target rows are the prior plus the term, rounded once; weight 0.5; the loss tensor
    accumulates.  accumulate = 0 overwrites."""
    name = 'b2_k6_c64_33x33'
    sides = case_inputs(name)
    hw, c = 33 * 33, 64
    gen = torch.Generator().manual_seed(7)
    r, e, e2 = reference(name, sides)
    prior = (torch.randn(4 * hw, c, generator=gen) * e['rows_b'].abs().max()).bfloat16()
    assert torch.isfinite(prior.float()).all()
    buf = prior.cuda()
    acc = torch.full((1,), 2.0, device='cuda')
    loss, ra, rb = run(sides, weight=0.5, bufs=[None, buf[2 * hw:]], accumulate=True, loss=acc)
    assert loss == pytest.approx(2.0 + 0.5 * e['loss'], rel=1e-6)
    assert torch.equal(buf[:2 * hw].cpu().view(torch.int16), prior[:2 * hw].view(torch.int16))
    pe = dca_emulated(sides, weight=0.5, prior=(None, prior[2 * hw:]))
    pe2 = dca_emulated(sides, weight=0.5, prior=(None, prior[2 * hw:]), reverse=True)
    tb = tight_bounds(pe, pe2, c, 'cov')
    # the term is small against the prior it joins: the bf16 flips are counted on the sum
    t_g = relnorm(rb, pe['grad_b'])
    print('accumulate: rows against the emulation', t_g, 'bound', tb['rows'])
    assert t_g <= tb['rows']
    assert not torch.equal(rb, prior[2 * hw:])
    buf2 = prior.cuda()
    _, _, rb2 = run(sides, weight=0.5, bufs=[None, buf2[2 * hw:]], accumulate=False)
    _, _, rb3 = run(sides, weight=0.5, want=(False, True))
    assert torch.equal(rb2, rb3) and torch.equal(buf2[:2 * hw].cpu().view(torch.int16), prior[:2 * hw].view(torch.int16))
    assert relnorm(rb3, dca_emulated(sides, weight=0.5)['grad_b']) <= tb['rows']


def test_feature_view_weight_and_wide_rows():
    """the features of both sides are a batch slice AND a channel slice of one larger tensor, read in place: bit-identical
    to the contiguous copy; weight 0.25; gradient rows of 72 columns whose last 8 stay"""
    from regda_amd import ops
    (fa, pa), (fb, pb) = make_inputs(2, 6, 64, 5, 7, 1.0, 3.0, 61)
    big = torch.randn(6, 128, 5, 7, generator=torch.Generator().manual_seed(3))
    big[1:3, 32:96], big[3:5, 32:96] = fa, fb
    bg = big.cuda()
    va, vb = bg[1:3, 32:96], bg[3:5, 32:96]
    assert not va.is_contiguous() and va.data_ptr() != bg.data_ptr()
    sides = ((fa, pa), (fb, pb))
    for kind in ('cov', 'mse'):
        want = run(sides, kind=kind, weight=0.25)
        got = run(((va, tuple(p.cuda() for p in pa)), (vb, tuple(p.cuda() for p in pb))), kind=kind, weight=0.25)
        assert got[0] == want[0] and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), kind
        r, e, e2 = reference('view', sides, kind=kind)
        ew = dca_emulated(sides, kind=kind, weight=0.25)
        tb = tight_bounds(e, e2, 64, kind)
        assert abs(got[0] - ew['loss']) / abs(ew['loss']) <= tb['loss']
        assert relnorm(got[1], ew['grad_a']) <= tb['rows'] and relnorm(got[2], ew['grad_b']) <= tb['rows']
    fill = torch.full((70, 72), 3.0, dtype=BF)
    wide = [fill.clone().cuda(), fill.clone().cuda()]
    ops.dca_loss(va, tuple(p.cuda() for p in pa), vb, tuple(p.cuda() for p in pb), weight=0.25, dfeat_a=wide[0], dfeat_b=wide[1])
    got = run(sides, kind='cov', weight=0.25)
    for s in range(2):
        assert torch.equal(wide[s].cpu()[:, :64], got[1 + s]) and torch.equal(wide[s].cpu()[:, 64:], fill[:, 64:])


NAN_SEED = 2          # tests/test_dca_cpu.py asserts that this seed's float64 diagonal has an entry below -0.01


def test_unstructured_inputs_give_a_nan_loss():
    """randn features and logits: a diagonal entry of R is negative (tests/test_dca_cpu.py asserts it in float64) and
    the loss is NaN, as in the reference"""
    loss, _, _ = run(random_inputs(2, 6, 64, 8, 8, NAN_SEED))
    assert np.isnan(loss)


def test_two_calls_are_bit_identical():
    for name in ('b2_k6_c32_5x7', 'b2_k6_c64_33x33', 'b4_k6_c2048_16x16'):
        sides = tuple(cuda_side(s) for s in case_inputs(name))
        for kind in ('cov', 'mse'):
            a, b = run(sides, kind=kind), run(sides, kind=kind)
            assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (name, kind)


def _nchw(rows, b, h, w):
    return rows.float().view(b, h, w, -1).permute(0, 3, 1, 2)


def test_modules_through_autograd_equal_the_op():
    """ICR, CCR, MSE_intra, MSE_cross with both multi_layer forms: the value and the gradient (scaled by the incoming
    one) are those of the op; CCR / MSE_cross give the source features no gradient; get_context, get_cross_corcoef_mat
    and regularize reproduce the cov loss"""
    from regda_amd import dca_modules as M
    name = 'b2_k6_c32_5x7'
    (fa, pa), (fb, pb) = case_inputs(name)
    h, w = 5, 7
    for multi in (True, False):
        pk = 'logits2' if multi else 'logits'
        qa, qb = (pa, pb) if multi else (pa[:1], pb[:1])
        sides = ((fa, qa), (fb, qb))
        for kind, intra, cross in (('cov', M.ICR, M.CCR), ('mse', M.MSE_intra, M.MSE_cross)):
            extra = (6,) if kind == 'cov' else ()
            loss, ra, rb = run(sides, pk, kind)
            x = torch.cat([fa, fb]).cuda().requires_grad_(True)
            out = intra((*(torch.cat([a, b]).cuda() for a, b in zip(qa, qb)), x), *extra, multi_layer=multi, ignore_bg=True)
            (3.0 * out).backward()
            assert out.item() == loss
            assert torch.equal(x.grad.cpu(), 3.0 * torch.cat([_nchw(ra, 2, h, w), _nchw(rb, 2, h, w)]))
            xs, xt = fa.cuda().requires_grad_(True), fb.cuda().requires_grad_(True)
            out = cross((*(p.cuda() for p in qa), xs), (*(p.cuda() for p in qb), xt), *extra, multi_layer=multi, ignore_bg=True)
            out.backward()
            assert out.item() == loss and xs.grad is None and torch.equal(xt.grad.cpu(), _nchw(rb, 2, h, w))
    m = M.CategoryAlign_Module(num_classes=6, ignore_bg=True)
    Pa, Pb = (probs(p, 'logits2', torch.float32).view(2, 6, h, w).cuda() for p in (pa, pb))
    R = m.get_cross_corcoef_mat(Pa, fa.cuda(), Pb, fb.cuda())
    r = dca_restated(((fa, pa), (fb, pb)))
    assert relnorm(R.cpu(), r['R']) <= 1e-5
    assert m.regularize(R).item() == pytest.approx(r['loss'], rel=1e-4)
    assert relnorm(m.get_context(Pa, fa.cuda()).cpu(), r['u_a']) <= 1e-5


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return (a @ b / (a.norm() * b.norm())).item()


WD = 100.0        # the term's weight in the step test (see its docstring)


def test_align_step_dca_weight_matches_the_composed_oracle(monkeypatch):
    """AlignStep(dca_weight=w) with step.dca['kind'] = 'mse' against the composed oracle: the CPU stage-2 step
    (oracle.step.CpuAlignStep) with oracle.model.forward wrapped to record (x1, x2, feat) of both domains and its second
    prototype_contrastive_loss call wrapped to add 2 w * (MSE_cross(src, tgt) + MSE_intra(src) + MSE_intra(tgt)), the
    definition of tests/dca_ref.py on the oracle's own fp32 tensors (the predictions and, for the cross term, the source
    features detached); the step halves that sum.

    Shape: the smallest the align tests use (2 + 2 tiles of 128^2, 8 x 8 feature pixels per image, 2048 channels,
    resnet17t); the intra terms compare one image with the other.

    kind 'mse' only.  The cov kind needs a correlation matrix with a positive diagonal; on an untrained network no class
    is separated, and on the CPU the oracle's own R failed the conditions of dca_ref.check_cov_conditions for every one
    of the eight model seeds 6 .. 13 (batch seed 11) in at least two of the three terms: minimum diagonal entries between
    -0.17 and 0.044, a NaN loss in 21 of the 24 matrices.  The cov kind is covered at op level.

    The mse term of an untrained network is about 1.17 (three terms of about 0.39) against a gradient norm of 119
    without it; on the CPU the oracle's norm is 119.4 with w = 1, 314 with w = 100: with w = 100 the norms with and
    without the term are asserted to differ by >= 1.5, so a missing, halved or doubled term moves the norm outside the
    0.06 of the stage-2 step tests.  The term's own gradient (the flat gradient with the term minus the one without,
    before clipping) is compared with the oracle's difference: cosines > 0.9 and norm within 0.12, the bounds and
    reasoning of test_align_step_triplet_weight; loss_dca rel 0.05 as loss_triplet there.  The updated weights: the
    classifier's update within 0.08 and the update directions' cosines, as tests/test_align_gpu.py asserts them.
    dca_weight = 0 is bit-identical to a step built without the argument."""
    from dca_ref import dca_differentiable
    from oracle import labelpath, model as omodel
    from oracle.step import CpuAlignStep
    from regda_amd.align import AlignStep
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.synthetic import make_batch
    rt, wd = 'resnet17t', WD
    sd = omodel.init_state_dict(rt, 6, seed=6)
    b = make_batch(b=2, size=128, seed=11, device='cpu')
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(1))
    ones = torch.ones(2, 512)
    gb = {k: v.cuda() for k, v in b.items()}
    keys = ('encoder.resnet.layer4.1.conv3.weight', 'encoder.resnet.layer1.0.conv1.weight', 'encoder.resnet.conv1.weight')

    def run_step(**kw):
        m = Deeplabv2(dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True, cascade=False,
                           use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048, num_classes=6,
                           is_ins_norm=True))
        m.load_state_dict(sd, strict=True)
        m.set_drop_masks(ones, ones)
        st = AlignStep(m, protos, **kw)
        assert st.dca == dict(kind='cov', ccr=True, icr=True, ignore_bg=True)
        st.dca['kind'] = 'mse'
        out = st.step(gb['images_s'], gb['label_s'], gb['images_t'], gb['regs_t'], 1e-3)
        torch.cuda.synchronize()
        views = {k: m._gviews[k].detach().float().cpu().clone() for k in keys}
        return st, out, m.flat_g.clone(), views, {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    st, (_, _, gn), g_on, v_on, w_on = run_step(dca_weight=wd)
    _, (_, _, gn_def), g_def, v_def, w_def = run_step()
    st0, _, g_zero, _, w_zero = run_step(dca_weight=0.0)
    assert torch.equal(g_zero, g_def) and st0.loss_dca.item() == 0.0
    for k in w_def:
        assert torch.equal(w_zero[k], w_def[k]), k

    fwd, pcl, outs, calls, terms = omodel.forward, labelpath.prototype_contrastive_loss, [], [], []

    def forward_recorded(*a, **k):
        outs.append(fwd(*a, **k))
        return outs[-1]

    def pcl_plus_dca(prototypes, feat, label, *a, **k):
        calls.append(label)
        v = pcl(prototypes, feat, label, *a, **k)
        if len(calls) == 2:
            (s1, s2, fs), (t1, t2, ft) = outs
            assert feat is ft
            Ps = probs((s1.detach(), s2.detach()), 'logits2', torch.float32)
            Pt = probs((t1.detach(), t2.detach()), 'logits2', torch.float32)
            term = dca_differentiable(fs.detach(), Ps, ft, Pt, 'mse', True)
            for f, P in ((fs, Ps), (ft, Pt)):
                term = term + dca_differentiable(f[:1], P[:1], f[1:], P[1:], 'mse', True)
            terms.append(term.item())
            v = v + 2 * wd * term
        return v

    def oracle():
        return CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, proto_decay=0.999).step(
            b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))
    ref0 = oracle()
    monkeypatch.setattr(omodel, 'forward', forward_recorded)
    monkeypatch.setattr(labelpath, 'prototype_contrastive_loss', pcl_plus_dca)
    cpu = CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, proto_decay=0.999)
    ref = cpu.step(b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))
    monkeypatch.undo()
    assert len(calls) == 2 and len(outs) == 2 and len(terms) == 1
    print('oracle: grad norm', ref['grad_norm'], 'without the term', ref0['grad_norm'], 'term', terms[0])
    assert ref['grad_norm'] >= 1.5 * ref0['grad_norm']
    want = wd * terms[0]
    print('loss_dca', st.loss_dca.item(), want, 'grad norm', gn.sqrt().item(), ref['grad_norm'])
    assert want > 0.0 and st.loss_dca.item() == pytest.approx(want, rel=0.05)
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)
    assert gn_def.sqrt().item() == pytest.approx(ref0['grad_norm'], rel=0.06)

    ref_delta = {k: ref['grads'][k] - ref0['grads'][k] for k in ref['grads']}
    ref_delta_norm = torch.sqrt(sum((v.double() ** 2).sum() for v in ref_delta.values())).item()
    delta_norm = (g_on.double() - g_def.double()).norm().item()
    print('the term alone', delta_norm, ref_delta_norm)
    assert delta_norm == pytest.approx(ref_delta_norm, rel=0.12)
    for k in keys:
        c = _cos(v_on[k] - v_def[k], ref_delta[k])
        print(k, 'cosine of the term\'s gradient', c)
        assert c > 0.9, (k, c)

    for k, tol in (('encoder.resnet.layer4.1.conv3.weight', 0.97), ('encoder.resnet.conv1.weight', 0.9)):
        c = _cos(cpu.sd[k].detach() - sd[k], w_on[k] - sd[k])
        print(k, 'cosine of the update', c)
        assert c > tol, (k, c)
    k = 'layer5.conv_last.4.weight'
    d_ref, d_got = cpu.sd[k].detach() - sd[k], w_on[k] - sd[k]
    assert ((d_got - d_ref).norm() / d_ref.norm()).item() < 0.08
