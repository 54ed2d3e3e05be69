"""GPU: the region-overlap term (rgda_upsample_overlap) per element against the float64 restatement
(tests/overlap_ref.py) at the pipeline's edge shapes, for Dice, soft Jaccard and a focal-Tversky, one and two heads; the
all-ignored input, out-of-range labels, accumulate and repeatability, the call without gradients; the TverskyLoss
modules; and the steps' overlap_weight_s / overlap_weight_t eagerly, as a recorded plan, as a captured graph, with the
DACS mix, in the stage-1 and stage-2 steps and across a save / load.

Bounds are this pipeline's edge-shape bounds (tests/test_iast_gpu.py header): loss and index rel 1e-5, gradients rtol
1e-3 / atol 1e-4 x max |reference gradient|; the class counts are exact.  An fp32 evaluation of the restatement itself on
the CPU (overlap_ref.loss_and_grads(dtype=torch.float32), all 15 (C, shape) cases x 3 variants x 1 and 2 heads) deviates
from float64 by at most 1.2e-7 (loss, relative), 5.8e-7 (index, relative) and 3.3e-6 x max (gradient); the kernels were
seen at 4.0e-8, 8.4e-7 and 5.9e-7 x max over the same cases, so the pipeline's bounds stand as they are."""
import numpy as np
import pytest
import torch

import overlap_ref

pytestmark = pytest.mark.gpu


def _check(what, got, ref, heads):
    loss, index, present, g1, g2 = got
    rloss, rindex, rpresent, rgrads = ref
    assert present.cpu().tolist() == rpresent.tolist(), what
    loss, index = loss.cpu().double().numpy(), index.cpu().double().numpy()
    grads = [g1.cpu(), g2.cpu()] if heads == 2 else [(g1 + g2).cpu()]
    gerr = max(float((g.double() - r).abs().max() / r.abs().max()) for g, r in zip(grads, rgrads))
    lerr = abs(float(loss[0]) - float(rloss)) / abs(float(rloss))
    on = rpresent.numpy() > 0
    ierr = np.abs(index - rindex.numpy())[:, on] / np.abs(rindex.numpy())[:, on]
    print(f'[{what}] present {rpresent.tolist()} loss rel {lerr:.2e} index rel {ierr.max():.2e} gradient / max {gerr:.2e}')
    assert index.shape == (heads, len(on)) and not index[:, ~on].any(), what
    np.testing.assert_allclose(loss[0], float(rloss), rtol=1e-5, atol=0, err_msg=what)
    np.testing.assert_allclose(index, rindex.numpy(), rtol=1e-5, atol=0, err_msg=what)
    for g, r in zip(grads, rgrads):
        np.testing.assert_allclose(g.numpy(), r.numpy(), rtol=1e-3, atol=1e-4 * float(r.abs().max()), err_msg=what)


def _call(d, heads, variant='dice', label=None, **kw):
    from regda_amd import ops
    p1 = d['p'][0].cuda()
    p2 = d['p'][1].cuda() if heads == 2 else p1
    label = d['label'] if label is None else label
    return ops.upsample_overlap(p1, p2, label.cuda(), *overlap_ref.VARIANTS[variant], heads=heads, **kw)


@pytest.mark.parametrize('variant', sorted(overlap_ref.VARIANTS))
@pytest.mark.parametrize('heads', (1, 2))
@pytest.mark.parametrize('k', range(len(overlap_ref.CASE_SHAPES)),
                         ids=lambda k: 'x'.join(map(str, overlap_ref.CASE_SHAPES[k][1])))
@pytest.mark.parametrize('C', overlap_ref.CLASSES)
def test_every_element_against_the_restatement(C, k, heads, variant):
    d = overlap_ref.case(C, k)
    got = _call(d, heads, variant)
    _check(f'c{C} {d["lo"]}->{d["hi"]} {variant} heads {heads}', got, overlap_ref.case_reference(d, heads, variant), heads)


def test_weight_scales_the_gradient_only():
    d = overlap_ref.case(7, 0)
    got = _call(d, 2, 'tversky', weight=0.37)
    _check('weight', got, overlap_ref.case_reference(d, 2, 'tversky', weight=0.37), 2)
    assert torch.equal(got[0], _call(d, 2, 'tversky')[0])
    zero = _call(d, 2, 'tversky', weight=0.0)
    assert torch.equal(zero[0], got[0]) and not zero[3].any() and not zero[4].any()


def test_everything_ignored_is_exactly_zero_and_leaves_accumulated_buffers_alone():
    d = overlap_ref.case(6, 0)
    label = torch.full_like(d['label'], -1)
    loss, index, present, g1, g2 = _call(d, 2, 'tversky', label=label)
    assert not loss.any() and not index.any() and not present.any() and not g1.any() and not g2.any()
    g = torch.Generator().manual_seed(2)
    prior1, prior2 = torch.randn(g1.shape, generator=g).cuda(), torch.randn(g2.shape, generator=g).cuda()
    prior1[0, 0, 0, :3] = 0.0
    prior2[0, 0, 0, :3] = -0.0
    a1, a2 = prior1.clone(), prior2.clone()
    loss, *_ = _call(d, 2, 'tversky', label=label, g1=a1, g2=a2, accumulate=True)
    assert not loss.any()
    assert torch.equal(a1.view(torch.int32), prior1.view(torch.int32)) and torch.equal(a2.view(torch.int32), prior2.view(torch.int32))


def test_out_of_range_label_is_ignored_and_sets_the_flag():
    d = overlap_ref.case(6, 3)
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    _call(d, 2, flag=flag)
    assert int(flag) == 0
    where = [(1, 17, 30), (0, 63, 63)]
    assert all(int(d['label'][w]) >= 0 for w in where)
    for value in (6, 255, -7, 1 << 40):
        bad, ignored = d['label'].clone(), d['label'].clone()
        for w in where:
            bad[w], ignored[w] = value, -1
        flag.zero_()
        got = _call(d, 2, label=bad, flag=flag)
        assert int(flag) == 1, value
        flag.zero_()
        want = _call(d, 2, label=ignored, flag=flag)
        assert int(flag) == 0
        for a, b in zip(got, want):
            assert torch.equal(a, b), value
    _check('ignored', want, overlap_ref.loss_and_grads(d['p'], ignored, *overlap_ref.VARIANTS['dice']), 2)
    # another ignore_label: the old one is then out of range
    flag.zero_()
    got = _call(d, 2, label=torch.where(d['label'] < 0, 255, d['label']), ignore_label=255, flag=flag)
    assert int(flag) == 0 and all(torch.equal(a, b) for a, b in zip(got, _call(d, 2)))
    _call(d, 2, ignore_label=255, flag=flag)
    assert int(flag) == 1


def test_accumulate_is_one_f32_add_and_runs_repeat_bit_for_bit():
    d = overlap_ref.case(7, 4)
    runs = [_call(d, 2, 'tversky', weight=0.3) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    loss, index, present, g1, g2 = runs[0]
    assert g1.abs().sum() > 0 and g2.abs().sum() > 0 and loss[0] > 0
    g = torch.Generator().manual_seed(5)
    prior1, prior2 = torch.randn(g1.shape, generator=g).cuda() * 1e-3, torch.randn(g2.shape, generator=g).cuda() * 1e-3
    a1, a2 = prior1.clone(), prior2.clone()
    loss_a, index_a, present_a, r1, r2 = _call(d, 2, 'tversky', weight=0.3, g1=a1, g2=a2, accumulate=True)
    assert r1 is a1 and r2 is a2
    assert torch.equal(loss_a, loss) and torch.equal(index_a, index) and torch.equal(present_a, present)
    assert torch.equal(a1, prior1 + g1) and torch.equal(a2, prior2 + g2)


@pytest.mark.parametrize('heads', (1, 2))
def test_without_gradients_the_same_outputs(heads):
    from regda_amd import ops
    d = overlap_ref.case(16, 1)
    full = _call(d, heads, 'jaccard')
    loss, index, present, g1, g2 = _call(d, heads, 'jaccard', want_grad=False)
    assert g1 is None and g2 is None
    assert torch.equal(loss, full[0]) and torch.equal(index, full[1]) and torch.equal(present, full[2])
    p = d['p'][0].cuda()
    with pytest.raises(ValueError, match='expected int64'):
        ops.upsample_overlap(p, p, d['label'].int().cuda())
    with pytest.raises(ValueError, match='gamma'):
        ops.upsample_overlap(p, p, d['label'].cuda(), gamma=0.5)
    with pytest.raises(ValueError, match='weight'):
        ops.upsample_overlap(p, p, d['label'].cuda(), weight=-1.0)


@pytest.mark.parametrize('heads', (1, 2))
def test_module_backward_is_the_ops_gradient_times_the_upstream_scalar(heads):
    from regda_amd import ops
    from regda_amd.gast import DiceLoss, JaccardLoss, TverskyLoss
    d = overlap_ref.case(7, 0)
    label = d['label'].cuda()
    for mod, prm in ((TverskyLoss(0.3, 0.7, gamma=1.5, smooth=1.0), overlap_ref.VARIANTS['tversky']),
                     (DiceLoss(), overlap_ref.VARIANTS['dice']), (JaccardLoss(), overlap_ref.VARIANTS['jaccard'])):
        ps = [p.cuda().requires_grad_(True) for p in d['p'][:heads]]
        total = mod(ps if heads == 2 else ps[0], label)
        (total * 3.0).backward()
        loss, index, present, g1, g2 = ops.upsample_overlap(ps[0].detach(), ps[-1].detach(), label, *prm, heads=heads)
        assert torch.equal(total.detach(), loss[0]) and torch.equal(mod.index, index) and torch.equal(mod.present, present)
        assert mod.index.is_cuda and mod.present.is_cuda and mod.flag_value() == 0
        want = [g1, g2] if heads == 2 else [g1 + g2]
        for p, g in zip(ps, want):
            assert torch.equal(p.grad, 3.0 * g)
        assert float(total.detach()) == pytest.approx(float(overlap_ref.loss_and_grads(d['p'][:heads], d['label'], *prm)[0]),
                                                      rel=1e-5)


# ------------------------------------------------------------------------------------------------- the steps
PRM = dict(alpha=0.3, beta=0.7, gamma=1.5, smooth=1.0)
W_S, W_T = 0.6, 0.4
ON = dict(overlap_weight_s=W_S, overlap_weight_t=W_T, overlap=PRM)
KEEP = ('s1', 's2', 't1', 't2', 'g1_s', 'g2_s', 'g1_t', 'g2_t')


def _shallow():
    from test_losses_gpu import _shallow as shallow
    rt, sd, b, protos, ones, model = shallow()
    return {k: v.cuda() for k, v in b.items()}, protos, ones, model


def _args(g):
    return g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t']


def _terms(st):
    return [t.clone() for t in (st.loss_overlap_s, st.overlap_index_s, st.overlap_present_s, st.loss_overlap_t,
                                st.overlap_index_t, st.overlap_present_t)]


def test_step_with_weight_zero_is_the_step_without_the_option():
    """Both weights 0: the same launches (the rows of a recorded plan) and the same bits."""
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    outs = []
    for kw in ({}, dict(overlap_weight_s=0.0, overlap_weight_t=0.0, overlap=PRM)):
        m = model()
        st = SSLStep(m, protos, **kw)
        o1 = [x.clone() for x in st.step(*_args(g), 1e-3)]
        stats = st.record_plan(*_args(g))
        outs.append((o1, [x.clone() for x in st._out], m.flat_p.clone(), stats))
        for side in 'st':
            assert all(getattr(st, name + side) is None for name in ('loss_overlap_', 'overlap_index_', 'overlap_present_'))
        assert st.overlap_flag_value() == 0
    (a1, a2, pa, sa), (b1, b2, pb, sb) = outs
    assert sa == sb
    for x, y in zip(a1 + a2 + [pa], b1 + b2 + [pb]):
        assert torch.equal(x, y)


def test_step_terms_their_gradients_and_the_recorded_plan():
    """loss_overlap_s / _t against the op and the restatement on the step's own logits and labels; the logit gradients
    are the weight-0 step's plus the op's own (one f32 add); the recorded plan gives the eager step's bits."""
    from regda_amd import ops
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    steps = {}
    for on in (False, True):
        m = model()
        st = SSLStep(m, protos, **(ON if on else {}))
        st.keep_debug = True
        out = [x.clone() for x in st.step(*_args(g), 1e-3)]
        steps[on] = (st, m, out, {k: st.debug[k].clone() for k in KEEP}, st.last_hard.clone())
    (st0, m0, out0, d0, hard0), (st1, m1, out1, d1, hard1) = steps[False], steps[True]
    assert all(torch.equal(d0[k], d1[k]) for k in ('s1', 's2', 't1', 't2')) and torch.equal(hard0, hard1)
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])      # the reported losses are the plain ones
    assert not torch.equal(m0.flat_p, m1.flat_p) and st1.overlap_flag_value() == 0
    prm = tuple(PRM[k] for k in ('alpha', 'beta', 'gamma', 'smooth'))
    for side, weight, label in (('s', W_S, g['label_s']), ('t', W_T, hard1)):
        x1, x2 = d1[side + '1'], d1[side + '2']
        loss, index, present, r1, r2 = ops.upsample_overlap(x1, x2, label, *prm, weight=weight)
        mine = [getattr(st1, name + side) for name in ('loss_overlap_', 'overlap_index_', 'overlap_present_')]
        assert all(t.is_cuda for t in mine)
        assert torch.equal(mine[0], loss) and torch.equal(mine[1], index) and torch.equal(mine[2], present)
        assert r1.abs().sum() > 0 and r2.abs().sum() > 0
        assert torch.equal(d1['g1_' + side], d0['g1_' + side] + r1) and torch.equal(d1['g2_' + side], d0['g2_' + side] + r2)
        ref = overlap_ref.loss_and_grads([x1.cpu(), x2.cpu()], label.cpu(), *prm, weight=weight)
        assert (ref[2] > 0).sum() >= 2
        _check('step ' + side, (loss, index, present, r1, r2), ref, 2)
    # step 2 eagerly and as the recording of a plan, then a replay against a third eager step
    m2 = model()
    st2 = SSLStep(m2, protos, **ON)
    st2.step(*_args(g), 1e-3)
    st1.keep_debug = False
    eager = [[x.clone() for x in st1.step(*_args(g), 1e-3)] + _terms(st1) for _ in range(2)]
    st2.record_plan(*_args(g), lr=1e-3)
    planned = [[x.clone() for x in st2._out] + _terms(st2)]
    planned.append([x.clone() for x in st2.step(*_args(g), 1e-3)] + _terms(st2))
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
        outs = []
        for _ in range(2):
            outs += [x.clone() for x in st.step(*_args(g), 1e-3)] + _terms(st)
        torch.cuda.synchronize()
        runs.append(outs + [m.flat_p.clone()])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert float(runs[0][3]) > 0 and float(runs[0][6]) > 0


def test_with_the_dacs_mix_the_target_term_reads_the_pasted_labels():
    from regda_amd import ops
    from regda_amd.aug.mix import DomainMix
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    st = SSLStep(model(), protos, mix=DomainMix('dacs', 6, seed=3), **ON)
    st.keep_debug = True
    st.step(*_args(g), 1e-3)
    d = st.debug
    assert st.last_mix is not None, 'this seed mixes the first batch'
    pasted, clean = st.last_hard, d['hard_clean']
    assert not torch.equal(pasted, clean)
    prm = tuple(PRM[k] for k in ('alpha', 'beta', 'gamma', 'smooth'))
    loss, index, present, _, _ = ops.upsample_overlap(d['t1'], d['t2'], pasted, *prm, weight=W_T)
    assert torch.equal(loss, st.loss_overlap_t) and torch.equal(index, st.overlap_index_t)
    assert torch.equal(present, st.overlap_present_t)
    other = ops.upsample_overlap(d['t1'], d['t2'], clean, *prm, weight=W_T)
    assert not torch.equal(other[2], present) and not torch.equal(other[0], loss)
    ref = overlap_ref.loss_and_grads([d['t1'].cpu(), d['t2'].cpu()], pasted.cpu(), *prm)
    assert present.cpu().tolist() == ref[2].tolist()
    np.testing.assert_allclose(float(loss), float(ref[0]), rtol=1e-5, atol=0)


def test_the_other_steps_take_the_source_term_and_refuse_the_target_term_by_name():
    from regda_amd import ops
    from regda_amd.align import AlignStep
    from regda_amd.source import SourceStep
    g, protos, ones, model = _shallow()
    prm = tuple(PRM[k] for k in ('alpha', 'beta', 'gamma', 'smooth'))
    makes = ((lambda m, **kw: SourceStep(m, **kw), lambda st: st.step(g['images_s'], g['label_s'], None, 1e-3)),
             (lambda m, **kw: AlignStep(m, protos, **kw),
              lambda st: st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], 1e-3)))
    for make, run in makes:
        with pytest.raises(NotImplementedError, match='overlap_weight_t'):
            make(None, overlap_weight_t=0.5)
        outs = []
        for kw in ({}, dict(overlap_weight_s=W_S, overlap=PRM)):
            m = model()
            st = make(m, **kw)
            outs.append(([x.clone() for x in run(st)], m.flat_p.clone(), st))
        (o0, p0, st0), (o1, p1, st1) = outs
        assert torch.equal(o0[0], o1[0]) and not torch.equal(p0, p1)       # the plain source loss; another update
        assert st0.loss_overlap_s is None and st1.loss_overlap_t is None and st1.overlap_flag_value() == 0
        assert st1.loss_overlap_s.is_cuda and 0 < float(st1.loss_overlap_s) < 1
        assert tuple(st1.overlap_index_s.shape) == (2, 6) and int(st1.overlap_present_s.sum()) == int((g['label_s'] >= 0).sum())


def test_save_and_load_continue_with_the_bits_of_the_uninterrupted_run():
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    m = model()
    st = SSLStep(m, protos, **ON)
    st.step(*_args(g), 1e-3)
    sd = st.state_dict()
    second = [x.clone() for x in st.step(*_args(g), 1e-3)] + _terms(st) + [m.flat_p.clone()]
    m2 = model()
    st2 = SSLStep(m2, protos + 1.0, **ON)           # other prototypes: everything comes from the state
    st2.load_state_dict(sd)
    resumed = [x.clone() for x in st2.step(*_args(g), 1e-3)] + _terms(st2) + [m2.flat_p.clone()]
    for x, y in zip(second, resumed):
        assert torch.equal(x, y)
