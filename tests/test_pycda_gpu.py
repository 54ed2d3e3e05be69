"""GPU: the PyCDA region pyramid term (rgda_upsample_pycda) per element against the float64 restatement
(tests/pycda_ref.py) at edge shapes; threshold ties, the all-inactive input, accumulate and repeatability, out-of-contract
soft labels; the PyramidCurriculumLoss module; SSLStep(pycda_weight=) eager, as a recorded plan, as a captured graph and
with the DACS mix.

Bounds are this pipeline's edge-shape bounds (tests/test_iast_gpu.py header): loss rel 1e-5, gradients rtol 1e-3 / atol
1e-4 x max |reference gradient|; an fp32 evaluation of the restatement itself deviates from float64 by at most 5e-8 (loss)
and 2.5e-7 x max (gradient) on the first three shapes.  The region counts are exact."""
import numpy as np
import pytest
import torch

import pycda_ref
from test_pycda_cpu import tie_soft

pytestmark = pytest.mark.gpu


def _check(what, got, ref, heads):
    loss, n_active, g1, g2 = got
    rloss, rn, rgrads = ref
    assert n_active.cpu().tolist() == rn, what
    loss = loss.cpu().double().numpy()
    grads = [g1.cpu(), g2.cpu()] if heads == 2 else [(g1 + g2).cpu()]
    gerr = max(float((g.double() - r).abs().max() / r.abs().max()) for g, r in zip(grads, rgrads))
    lerr = np.abs(loss - rloss.numpy()) / np.where(rloss.numpy() == 0, 1.0, np.abs(rloss.numpy()))
    print(f'[{what}] n_active {rn} loss rel {lerr.max():.2e} gradient / max {gerr:.2e}')
    for l in range(len(rn)):
        if rn[l] == 0:
            assert loss[1 + l] == 0.0, what
    np.testing.assert_allclose(loss, rloss.numpy(), rtol=1e-5, atol=0, err_msg=what)
    for g, r in zip(grads, rgrads):
        np.testing.assert_allclose(g.numpy(), r.numpy(), rtol=1e-3, atol=1e-4 * float(r.abs().max()), err_msg=what)


@pytest.mark.parametrize('heads', (1, 2))
@pytest.mark.parametrize('k', range(len(pycda_ref.CASE_SHAPES)), ids=lambda k: 'x'.join(map(str, pycda_ref.CASE_SHAPES[k][1])) +
                         '-' + '.'.join(map(str, pycda_ref.CASE_SHAPES[k][2])))
@pytest.mark.parametrize('C', pycda_ref.CLASSES)
def test_every_element_against_the_restatement(C, k, heads):
    from regda_amd import ops
    d = pycda_ref.case(C, k)
    p1 = d['p'][0].cuda()
    p2 = d['p'][1].cuda() if heads == 2 else p1
    got = ops.upsample_pycda(p1, p2, d['soft'].cuda(), d['sizes'], heads=heads)
    _check(f'c{C} {d["lo"]}->{d["hi"]} sizes {d["sizes"]} heads {heads}', got, pycda_ref.case_reference(d, heads), heads)


def test_level_weights_threshold_and_weight_scale_the_terms():
    from regda_amd import ops
    d = pycda_ref.case(7, 0)
    lw, weight, thresh = (0.2, 1.5, 0.7), 0.37, 0.8
    ref = pycda_ref.loss_and_grads(d['p'], d['soft'], d['sizes'], thresh=thresh, level_weight=lw, weight=weight)
    assert ref[1] != pycda_ref.case_reference(d, 2)[1]          # another threshold, other active sets
    got = ops.upsample_pycda(d['p'][0].cuda(), d['p'][1].cuda(), d['soft'].cuda(), d['sizes'], thresh=thresh, level_weight=lw,
                             weight=weight)
    _check('weights', got, ref, 2)
    # without gradients: the same losses and counts
    loss, n, g1, g2 = ops.upsample_pycda(d['p'][0].cuda(), d['p'][1].cuda(), d['soft'].cuda(), d['sizes'], thresh=thresh,
                                         level_weight=lw, weight=weight, want_grad=False)
    assert g1 is None and g2 is None and torch.equal(loss, got[0]) and torch.equal(n, got[1])
    with pytest.raises(ValueError):
        ops.upsample_pycda(d['p'][0].cuda(), d['p'][1].cuda(), d['soft'].cuda(), (4, 12))
    with pytest.raises(ValueError, match='expected float32'):
        ops.upsample_pycda(d['p'][0].cuda(), d['p'][1].cuda(), d['soft'][:, :5].cuda(), (4, 0))


def test_threshold_ties_give_the_same_active_sets_on_the_device():
    """A region exactly at the threshold is inactive; one pixel raised by 2^-24 makes exactly that region active."""
    from regda_amd import ops
    p = [x.cuda() for x in pycda_ref.make_logits(1, 6, 3, 5, 3, heads=2)]
    loss0, n0, g1, g2 = ops.upsample_pycda(p[0], p[1], tie_soft().cuda(), (4, 0))
    assert n0.tolist() == [0, 0] and not loss0.any() and not g1.any() and not g2.any()
    bumped = tie_soft(bump=True)
    got = ops.upsample_pycda(p[0], p[1], bumped.cuda(), (4, 0))
    assert got[1].tolist() == [1, 1] == [t[3] for t in pycda_ref.targets(bumped, (4, 0))]
    _check('tie', got, pycda_ref.loss_and_grads([x.cpu() for x in p], bumped, (4, 0)), 2)
    # the gradient of level 0 lives in the one active square's footprint: other low-resolution corners stay exactly 0
    only0 = ops.upsample_pycda(p[0], p[1], bumped.cuda(), (4,))
    assert only0[1].tolist() == [1] and only0[2].abs().max() > 0 and not only0[2][0, :, 2, 0].any()


def test_all_inactive_input_is_exactly_zero_and_leaves_accumulated_buffers_alone():
    from regda_amd import ops
    C = 6
    p = [x.cuda() for x in pycda_ref.make_logits(2, C, 5, 7, 1)]
    soft = torch.full((2, C, 33, 45), 1.0 / C).cuda()
    loss, n, g1, g2 = ops.upsample_pycda(p[0], p[1], soft, (2, 8, 0))
    assert not n.any() and not loss.any() and not g1.any() and not g2.any()
    g = torch.Generator().manual_seed(2)
    prior1, prior2 = torch.randn(g1.shape, generator=g).cuda(), torch.randn(g2.shape, generator=g).cuda()
    prior1[0, 0, 0, :3] = 0.0
    a1, a2 = prior1.clone(), prior2.clone()
    ops.upsample_pycda(p[0], p[1], soft, (2, 8, 0), g1=a1, g2=a2, accumulate=True)
    assert torch.equal(a1.view(torch.int32), prior1.view(torch.int32)) and torch.equal(a2.view(torch.int32), prior2.view(torch.int32))


def test_accumulate_is_one_f32_add_and_runs_repeat_bit_for_bit():
    from regda_amd import ops
    d = pycda_ref.case(7, 0)
    p1, p2, soft = d['p'][0].cuda(), d['p'][1].cuda(), d['soft'].cuda()
    runs = [ops.upsample_pycda(p1, p2, soft, d['sizes'], weight=0.3) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    loss, n, g1, g2 = runs[0]
    assert g1.abs().sum() > 0 and g2.abs().sum() > 0 and loss[0] > 0
    g = torch.Generator().manual_seed(5)
    prior1, prior2 = torch.randn(g1.shape, generator=g).cuda() * 1e-3, torch.randn(g2.shape, generator=g).cuda() * 1e-3
    a1, a2 = prior1.clone(), prior2.clone()
    loss_a, n_a, r1, r2 = ops.upsample_pycda(p1, p2, soft, d['sizes'], weight=0.3, g1=a1, g2=a2, accumulate=True)
    assert r1 is a1 and r2 is a2 and torch.equal(loss_a, loss) and torch.equal(n_a, n)
    assert torch.equal(a1, prior1 + g1) and torch.equal(a2, prior2 + g2)


def test_out_of_contract_soft_sets_the_flag_and_is_clamped():
    from regda_amd import ops
    d = pycda_ref.case(6, 3)
    p1, p2 = d['p'][0].cuda(), d['p'][1].cuda()
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.upsample_pycda(p1, p2, d['soft'].cuda(), d['sizes'], flag=flag)
    assert int(flag) == 0
    for value in (1.5, -0.1, float('nan')):
        soft = d['soft'].clone()
        soft[1, 2, 17, 30] = value
        soft[0, 5, 32, 44] = value          # the last pixel of a clipped border square
        flag.zero_()
        got = ops.upsample_pycda(p1, p2, soft.cuda(), d['sizes'], flag=flag)
        assert int(flag) == 1, value
        want = ops.upsample_pycda(p1, p2, pycda_ref.clamp_soft(soft).cuda(), d['sizes'], flag=flag)
        for a, b in zip(got, want):
            assert torch.equal(a, b), value


@pytest.mark.parametrize('heads', (1, 2))
def test_module_backward_is_the_ops_gradient_times_the_upstream_scalar(heads):
    from regda_amd import ops
    from regda_amd.gast import PyramidCurriculumLoss
    d = pycda_ref.case(7, 0)
    lw = (0.5, 0.3, 0.2)
    soft = d['soft'].cuda()
    ps = [p.cuda().requires_grad_(True) for p in d['p'][:heads]]
    mod = PyramidCurriculumLoss(sizes=d['sizes'], thresh=0.5, level_weight=lw)
    total = mod(ps if heads == 2 else ps[0], soft)
    (total * 3.0).backward()
    loss, n, g1, g2 = ops.upsample_pycda(ps[0].detach(), ps[-1].detach(), soft, d['sizes'], level_weight=lw, heads=heads)
    assert torch.equal(total.detach(), loss[0]) and torch.equal(mod.last_levels, loss[1:]) and torch.equal(mod.last_active, n)
    assert mod.last_levels.is_cuda and mod.last_active.is_cuda and mod.flag_value() == 0
    want = [g1, g2] if heads == 2 else [g1 + g2]
    for p, g in zip(ps, want):
        assert torch.equal(p.grad, 3.0 * g)
    assert float(total.detach()) == pytest.approx(float(pycda_ref.loss_and_grads(d['p'][:heads], d['soft'], d['sizes'], level_weight=lw)[0][0]),
                                         rel=1e-5)


# ------------------------------------------------------------------------------------------------- the step
SIZES = (8, 16, 32, 64, 0)
# the fixture's soft labels are confident per pixel but independent from pixel to pixel, so a region's mean sits near
# 1 / 6 for every class: a threshold just above it leaves active and inactive regions at the levels up to 64 (counted on
# the CPU on soft_t: 1024 of 1024, 252 of 256, 52 of 64, 1 of 16, 0 of 4; the refined label the step reads gave 1023, 256,
# 64, 16, 4), where the default 0.5 leaves none
THRESH = 0.175
ON = dict(pycda_weight=0.4, pycda_thresh=THRESH)


def _shallow():
    from test_losses_gpu import _shallow as shallow
    rt, sd, b, protos, ones, model = shallow()
    return {k: v.cuda() for k, v in b.items()}, protos, ones, model


def _args(g):
    return g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t']


def test_step_with_weight_zero_is_the_step_without_the_option():
    """pycda_weight = 0: the same launches (the rows of a recorded plan) and the same bits."""
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    outs = []
    for kw in ({}, dict(pycda_weight=0.0, pycda_sizes=(4, 0), pycda_thresh=0.3)):
        m = model()
        st = SSLStep(m, protos, **kw)
        o1 = [x.clone() for x in st.step(*_args(g), 1e-3)]
        stats = st.record_plan(*_args(g))
        outs.append((o1, [x.clone() for x in st._out], m.flat_p.clone(), stats))
        assert st.loss_pycda is None and st.pycda_flag_value() == 0
    (a1, a2, pa, sa), (b1, b2, pb, sb) = outs
    assert sa == sb
    for x, y in zip(a1 + a2 + [pa], b1 + b2 + [pb]):
        assert torch.equal(x, y)


def test_step_term_its_gradient_and_the_recorded_plan():
    """loss_pycda against the restatement on the step's own target logits and soft label; the logit gradient is the
    weight-0 step's plus the op's own (one f32 add); the recorded plan gives the eager step's bits."""
    from regda_amd import ops
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    weight = ON['pycda_weight']
    steps = {}
    for on in (False, True):
        m = model()
        st = SSLStep(m, protos, **(ON if on else {}))
        st.keep_debug = True
        out = [x.clone() for x in st.step(*_args(g), 1e-3)]
        steps[on] = (st, m, out, {k: v.clone() for k, v in st.debug.items() if k in ('t1', 't2', 'g1_t', 'g2_t', 'soft')})
    (st0, m0, out0, d0), (st1, m1, out1, d1) = steps[False], steps[True]
    assert all(torch.equal(d0[k], d1[k]) for k in ('t1', 't2', 'soft'))
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])      # the reported losses are the plain ones
    ref, rn, _ = pycda_ref.loss_and_grads([d1['t1'].cpu(), d1['t2'].cpu()], d1['soft'].cpu(), SIZES, thresh=THRESH)
    got = st1.loss_pycda.cpu().double()
    print(f'[step] loss_pycda {got.tolist()} restatement {ref.tolist()} n_active {rn}')
    assert st1.loss_pycda.shape == (1 + len(SIZES),) and st1.pycda_active.cpu().tolist() == rn and sum(rn) > 0
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-5, atol=0)
    assert st1.pycda_flag_value() == 0
    loss, n, r1, r2 = ops.upsample_pycda(d1['t1'], d1['t2'], d1['soft'], SIZES, thresh=THRESH, weight=weight)
    assert torch.equal(loss, st1.loss_pycda)
    assert r1.abs().sum() > 0 and torch.equal(d1['g1_t'], d0['g1_t'] + r1) and torch.equal(d1['g2_t'], d0['g2_t'] + r2)
    # step 2 eagerly and as the recording of a plan, then a replay against a third eager step
    m2 = model()
    st2 = SSLStep(m2, protos, **ON)
    st2.keep_debug = True
    st2.step(*_args(g), 1e-3)
    st1.keep_debug = st2.keep_debug = False
    eager = [[x.clone() for x in st1.step(*_args(g), 1e-3)] + [st1.loss_pycda.clone()] for _ in range(2)]
    st2.record_plan(*_args(g), lr=1e-3)
    planned = [[x.clone() for x in st2._out] + [st2.loss_pycda.clone()]]
    planned.append([x.clone() for x in st2.step(*_args(g), 1e-3)] + [st2.loss_pycda.clone()])
    for e, p in zip(eager, planned):
        for x, y in zip(e, p):
            assert torch.equal(x, y)
    assert torch.equal(m1.flat_p, m2.flat_p)
    assert not torch.equal(eager[0][3], eager[1][3])        # the term moves from step to step


def test_captured_graph_gives_the_eager_bits():
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    runs = []
    for captured in (False, True):
        m = model()
        m.set_drop_masks(ones.cuda(), ones.cuda())          # (device masks: nothing is copied from the host in capture)
        st = SSLStep(m, protos, loss_t='focal', **ON)
        st.step(*_args(g), 1e-3)
        if captured:
            st.capture(*_args(g))
        out = [x.clone() for x in st.step(*_args(g), 1e-3)] + [st.loss_pycda.clone(), st.pycda_active.clone()]
        torch.cuda.synchronize()
        runs.append(out + [m.flat_p.clone()])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert float(runs[0][3][0]) > 0


def test_with_the_dacs_mix_the_term_reads_the_pasted_copy():
    from regda_amd import ops
    from regda_amd.aug.mix import DomainMix
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    soft_in = g['soft_t'].clone()
    st = SSLStep(model(), protos, mix=DomainMix('dacs', 6, seed=3), refine_label=False, **ON)
    st.keep_debug = True
    st.step(*_args(g), 1e-3)
    d = st.debug
    assert st.last_mix is not None, 'this seed mixes the first batch'
    assert torch.equal(g['soft_t'], soft_in) and st.last_soft_t is g['soft_t']          # the caller's tensor is not written
    pasted = d['soft_loss']
    assert pasted.data_ptr() != g['soft_t'].data_ptr() and not torch.equal(pasted, soft_in)
    changed = (pasted != soft_in).any(1)        # where the paste changed something the label is one-hot
    assert changed.any() and bool((pasted.max(1).values[changed] == 1.0).all())
    loss, n, _, _ = ops.upsample_pycda(d['t1'], d['t2'], pasted, SIZES, thresh=THRESH, weight=0.4)
    assert torch.equal(loss, st.loss_pycda) and torch.equal(n, st.pycda_active)
    clean = ops.upsample_pycda(d['t1'], d['t2'], soft_in, SIZES, thresh=THRESH, weight=0.4)[0]
    assert not torch.equal(clean, st.loss_pycda)
    ref, rn, _ = pycda_ref.loss_and_grads([d['t1'].cpu(), d['t2'].cpu()], pasted.cpu(), SIZES, thresh=THRESH)
    assert st.pycda_active.cpu().tolist() == rn
    np.testing.assert_allclose(st.loss_pycda.cpu().double().numpy(), ref.numpy(), rtol=1e-5, atol=0)


def test_the_other_steps_refuse_the_option_by_name():
    from regda_amd.align import AlignStep
    from regda_amd.source import SourceStep
    with pytest.raises(NotImplementedError, match='pycda_weight'):
        AlignStep(None, None, pycda_weight=0.5)
    with pytest.raises(NotImplementedError, match='pycda_weight'):
        SourceStep(None, pycda_weight=0.5)
