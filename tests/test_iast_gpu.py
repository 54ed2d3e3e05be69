"""GPU: IAST self-training.  The entropy / KLD regularisers (rgda_upsample_reg) against the reference's own functions
(tests/golden/iast.npz) and against the CPU restatement (tests/iast_ref.py) in fp64 at edge shapes; the adaptive
pseudo-label stages (rgda_iast_hist / _percentile / _label), IASTSelector and generate_pseudo bit for bit against the
restatement and the reference's loop; SSLStep(ent_weight, kld_weight) eager, as a recorded plan and as a captured graph.

Bounds are the project's own for this pipeline: on the goldens loss rel 2e-6, gradients rtol 2e-4 / atol 1e-8
(tests/test_losses_gpu.py, tests/test_gdp_gpu.py); at the edge shapes loss rel 1e-5, gradients rtol 1e-3 /
atol 1e-4 x max |gradient|.  Everything of the selector is exact."""
import numpy as np
import pytest
import torch

import iast_ref

pytestmark = pytest.mark.gpu

ENT, KLD = 1, 2


def _close_or_nan(got, want, nan, **tol):
    if nan:
        assert np.isnan(got).all(), 'the reference gives NaN here'
    else:
        np.testing.assert_allclose(got, want, **tol)


# ------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize('kind', ('bin', 'frac', 'zero', 'neg'))
@pytest.mark.parametrize('C', (6, 7, 16))
def test_regularisers_match_the_reference_goldens(gold, C, kind):
    """entropyloss / kldloss (the drop-in autograd functions) and the raw entry point with both terms at once, on the
    reference's cases: loss and gradient against its fp64 results, NaN where it gives NaN (all-zero weights)."""
    from regda_amd import ops
    from regda_amd.utils.tools import entropyloss, kldloss
    g = gold('iast.npz')
    z = torch.from_numpy(g[f'reg/c{C}/logits']).float().cuda()
    w = torch.from_numpy(g[f'reg/c{C}/w_{kind}']).cuda()
    want = {n: (g[f'reg/c{C}/{kind}/{n}_loss64'], g[f'reg/c{C}/{kind}/{n}_grad64']) for n in ('ent', 'kld')}
    nan = kind == 'zero'
    for name, fn in (('ent', entropyloss), ('kld', kldloss)):
        for wt in (w, w[:, 0]):             # N x 1 x H x W and N x H x W
            x = z.clone().requires_grad_(True)
            loss = fn(x, wt)
            (loss * 3.0).backward()
            err = abs(float(loss.detach()) / float(want[name][0]) - 1)
            print(f'[c{C} {kind} {name}] loss {float(loss.detach()):.9g} (reference fp64 {float(want[name][0]):.9g}, fp32 '
                  f'{float(g[f"reg/c{C}/{kind}/{name}_loss32"]):.9g}) rel {err:.2e}')
            _close_or_nan(loss.detach().cpu().numpy(), want[name][0], nan, rtol=2e-6)
            _close_or_nan(x.grad.cpu().numpy() / 3.0, want[name][1], nan, rtol=2e-4, atol=1e-8)
    # both terms in one call, lambdas 0.7 / 1.9, one head: g1 + g2 is the gradient
    loss, g1, g2 = ops.upsample_reg(z, z, w_ent=w, w_kld=w, lambda_ent=0.7, lambda_kld=1.9, heads=1)
    _close_or_nan(loss.cpu().numpy(), np.array([want['ent'][0], want['kld'][0]]), nan, rtol=2e-6)
    _close_or_nan((g1 + g2).cpu().numpy(), 0.7 * want['ent'][1] + 1.9 * want['kld'][1], nan, rtol=2e-4, atol=1e-8)
    # the zero form of an empty region: exactly 0, gradient exactly 0
    if nan:
        loss, g1, g2 = ops.upsample_reg(z, z, w_ent=w, w_kld=w, heads=1, empty_is_zero=True)
        assert not loss.any() and not g1.any() and not g2.any()


# ------------------------------------------------------------------------------------------------- edge shapes
SHAPES = [((5, 7), (33, 45)), ((9, 11), (9, 11)), ((4, 4), (64, 64))]
MASKS = ('mixed', 'all_ignored', 'none_ignored', 'explicit')
_REF = {}


def reg_inputs(C, lo, hi):
    key = (C, lo, hi)
    if key not in _REF:
        g = torch.Generator().manual_seed(100 * C + lo[0] + hi[1])
        p1, p2 = torch.randn(2, C, *lo, generator=g) * 2.5, torch.randn(2, C, *lo, generator=g) * 2.5
        p1[0, :, 0, 0] = 0.0
        p2[1, 2, -1, -1] = 90.0         # saturated corner: the other probabilities underflow
        lab = torch.randint(0, C, (2, *hi), generator=g)
        lab = torch.where(torch.rand(2, *hi, generator=g) < 0.35, torch.full_like(lab, -1), lab)
        we = torch.rand(2, *hi, generator=g) * (torch.rand(2, *hi, generator=g) < 0.6)
        wk = torch.rand(2, *hi, generator=g) * 2 - 0.5          # some negative entries
        _REF[key] = dict(p1=p1, p2=p2, lab=lab, we=we, wk=wk, refs={})
    return _REF[key]


def reg_reference(d, mask, terms, heads, hi, lam):
    """(ent, kld, [gradient per head]) of the restatement in fp64 with the NaN form; computed once per case."""
    key = (mask, terms, heads)
    if key not in d['refs']:
        lab = {'mixed': d['lab'], 'all_ignored': torch.full_like(d['lab'], -1), 'none_ignored': d['lab'].clamp(min=0)}.get(mask)
        we, wk = (d['we'].double(), d['wk'].double()) if mask == 'explicit' else iast_ref.derived_weights(lab, -1, torch.float64)
        ps = [p.double().requires_grad_(True) for p in (d['p1'], d['p2'])[:heads]]
        out = {}
        for ez in (False, True):
            for p in ps:
                p.grad = None
            ent, kld, obj = iast_ref.reg(ps, hi, we if terms & ENT else None, wk if terms & KLD else None, lam[0], lam[1], ez)
            if obj.requires_grad:
                obj.backward()
            grads = [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in ps]
            out[ez] = (float(ent.detach()), float(kld.detach()), grads)
        d['refs'][key] = (lab, out)
    return d['refs'][key]


@pytest.mark.parametrize('heads', (1, 2))
@pytest.mark.parametrize('lo,hi', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('C', (6, 7, 16))
def test_regularisers_at_edge_shapes_against_the_restatement(C, lo, hi, heads):
    """Upsampled and plain (h == H) logits, one and two heads, derived masks (mixed, all ignored, none ignored) and
    explicit maps with negative entries, each term alone and both, empty_is_zero both ways -- against tests/iast_ref.py
    in fp64.  An empty region is NaN (loss and gradient) in the reference's form and exactly 0 in the zero form."""
    from regda_amd import ops
    d = reg_inputs(C, lo, hi)
    lam = (0.6, 1.7)
    p1, p2 = d['p1'].cuda(), (d['p2'] if heads == 2 else d['p1']).cuda()
    for mask in MASKS:
        for terms in (ENT, KLD, ENT | KLD):
            lab, refs = reg_reference(d, mask, terms, heads, hi, lam)
            kw = dict(w_ent=d['we'].cuda(), w_kld=d['wk'].cuda(), size=hi) if mask == 'explicit' else dict(label=lab.cuda())
            empty = {ENT: mask == 'none_ignored', KLD: mask == 'all_ignored'}
            for ez in (False, True):
                loss, g1, g2 = ops.upsample_reg(p1, p2, terms=terms, lambda_ent=lam[0], lambda_kld=lam[1], heads=heads,
                                                empty_is_zero=ez, **kw)
                loss, grads = loss.cpu().numpy(), ([g1.cpu(), g2.cpu()] if heads == 2 else [(g1 + g2).cpu()])
                rent, rkld, rgrads = refs[ez]
                what = f'c{C} {lo}->{hi} heads {heads} {mask} terms {terms} ez {ez}'
                any_nan = False
                for t, slot, ref in ((ENT, 0, rent), (KLD, 1, rkld)):
                    if not terms & t:
                        assert loss[slot] == 0.0, what
                    elif empty[t]:
                        any_nan |= not ez
                        assert (loss[slot] == 0.0) if ez else np.isnan(loss[slot]), what
                        assert (ref == 0.0) if ez else np.isnan(ref), what
                    else:
                        assert loss[slot] == pytest.approx(ref, rel=1e-5), what
                for got, ref in zip(grads, rgrads):
                    if any_nan:
                        assert torch.isnan(got).all() and torch.isnan(ref).all(), what
                    else:
                        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-3, atol=1e-4 * float(ref.abs().max()),
                                                   err_msg=what)
                if ez and all(empty[t] for t in (ENT, KLD) if terms & t):
                    assert all(not g.any() for g in grads), what         # exactly 0


def test_accumulate_is_one_f32_add_and_runs_repeat_bit_for_bit():
    from regda_amd import ops
    d = reg_inputs(7, (5, 7), (33, 45))
    p1, p2, lab = d['p1'].cuda(), d['p2'].cuda(), d['lab'].cuda()
    runs = [ops.upsample_reg(p1, p2, lab, lambda_ent=0.3, lambda_kld=0.2) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    loss, g1, g2 = runs[0]
    assert g1.abs().sum() > 0 and g2.abs().sum() > 0 and loss.min() > 0
    g = torch.Generator().manual_seed(5)
    prior1, prior2 = torch.randn(g1.shape, generator=g).cuda() * 1e-3, torch.randn(g2.shape, generator=g).cuda() * 1e-3
    a1, a2 = prior1.clone(), prior2.clone()
    loss_a, r1, r2 = ops.upsample_reg(p1, p2, lab, lambda_ent=0.3, lambda_kld=0.2, g1=a1, g2=a2, accumulate=True)
    assert r1 is a1 and r2 is a2 and torch.equal(loss_a, loss)
    assert torch.equal(a1, prior1 + g1) and torch.equal(a2, prior2 + g2)
    # a term that is off costs its slot and its gradient nothing: lambda is not looked at
    l_e, e1, _ = ops.upsample_reg(p1, p2, lab, terms=ENT, lambda_ent=0.3, lambda_kld=123.0)
    l_k, k1, _ = ops.upsample_reg(p1, p2, lab, terms=KLD, lambda_ent=123.0, lambda_kld=0.2)
    assert l_e[1] == 0 and l_k[0] == 0 and l_e[0] == loss[0] and l_k[1] == loss[1]
    torch.testing.assert_close(e1 + k1, g1, rtol=1e-5, atol=1e-9)
    # what the wrapper refuses itself: a derived mask without a label, a label of another shape
    with pytest.raises(ValueError, match='label'):
        ops.upsample_reg(p1, p2, terms=ENT, w_kld=d['wk'].cuda())
    with pytest.raises(ValueError, match='expected int64'):
        ops.upsample_reg(p1, p2, lab[:1])            # one image's labels for a batch of two
    with pytest.raises(ValueError, match='expected int64'):
        ops.upsample_reg(p1, p2, lab, size=(33, 44))
    # without gradients: the same losses
    assert torch.equal(ops.upsample_reg(p1, p2, lab, want_grad=False)[0], loss)


# ------------------------------------------------------------------------------------------------- selector stages
@pytest.mark.parametrize('kind', ('softmax', 'confident', 'fp16_ties', 'missing_class', 'class_ties'))
@pytest.mark.parametrize('H,W', ((7, 13), (64, 64)))
@pytest.mark.parametrize('C', (6, 16))
def test_iast_stages_equal_the_restatement_on_every_element(C, H, W, kind):
    from regda_amd import ops
    n = 2
    probs = iast_ref.selector_inputs(kind, n, C, H, W, seed=C + H)
    arg, maxp, h = iast_ref.hist(probs)
    ws = ops.iast_hist(torch.from_numpy(probs).cuda())
    g_hist, g_maxp, g_arg = ops.iast_views(ws, n, C, H, W)
    assert np.array_equal(g_arg.cpu().numpy(), arg)
    assert np.array_equal(g_maxp.cpu().numpy(), maxp)
    assert np.array_equal(g_hist.cpu().numpy(), h)
    rng = np.random.default_rng(C * H)
    prepend = np.round(rng.uniform(0.3, 1.0, C), 3)
    prepend[0], prepend[1] = 0.9, float(np.float16(0.75))       # the start value; a value that is itself an fp16
    q = rng.random(C)
    q[2], q[3], q[4] = 0.0, 1.0, (100 * (1 - 0.2 * 0.9 ** 8.0)) / 100
    want = np.array([iast_ref.percentile_from_hist(h[c], prepend[c], q[c]) for c in range(C)])
    got = ops.iast_percentile(ws, torch.from_numpy(prepend).cuda(), torch.from_numpy(q).cuda()).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want), (got, want)
    if kind == 'missing_class':
        assert got[1] == np.float32(prepend[1])
    thresh = 0.9 * prepend + 0.1 * want         # f64 thresholds, some of them inside the data
    lab = ops.iast_label(ws, torch.from_numpy(thresh).cuda(), n, H, W)
    assert lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy(), iast_ref.label_from(arg, maxp, thresh))
    # a second call on the same workspace starts from a cleared histogram
    ops.iast_hist(torch.from_numpy(probs).cuda(), ws=ws)
    assert np.array_equal(g_hist.cpu().numpy(), h)


def test_iast_stages_over_several_grid_strides():
    """3 x 6 x 512 x 512: 768 tiles for the 512 workgroups of the histogram pass and 3072 blocks of work for the 2048 of
    the label pass, so both walk their grid-stride loops more than once (and unevenly); every element as above."""
    from regda_amd import ops
    n, C, H, W = 3, 6, 512, 512
    probs = iast_ref.selector_inputs('softmax', n, C, H, W, seed=9)
    arg, maxp, h = iast_ref.hist(probs)
    ws = ops.iast_hist(torch.from_numpy(probs).cuda())
    g_hist, g_maxp, g_arg = ops.iast_views(ws, n, C, H, W)
    assert np.array_equal(g_arg.cpu().numpy(), arg) and np.array_equal(g_maxp.cpu().numpy(), maxp)
    assert np.array_equal(g_hist.cpu().numpy(), h) and int(h.sum()) == n * H * W
    prepend, q = np.full(C, 0.9), np.linspace(0.05, 0.95, C)
    want = np.array([iast_ref.percentile_from_hist(h[c], prepend[c], q[c]) for c in range(C)])
    got = ops.iast_percentile(ws, torch.from_numpy(prepend).cuda(), torch.from_numpy(q).cuda()).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    thresh = want.astype(np.float64)
    lab = ops.iast_label(ws, torch.from_numpy(thresh).cuda(), n, H, W).cpu().numpy()
    assert np.array_equal(lab, iast_ref.label_from(arg, maxp, thresh)) and 0 < (lab == 0).mean() < 1


@pytest.mark.parametrize('C', (6, 16))
def test_selector_reproduces_the_reference_loop_over_three_batches(gold, C):
    from regda_amd.utils.tools import IASTSelector
    g = gold('iast.npz')
    sel = IASTSelector(C, float(g['sel/alpha']), float(g['sel/beta']), float(g['sel/gamma']))
    for k in range(3):
        lab = sel.update(torch.from_numpy(g[f'sel/c{C}/probs'][k]).cuda())
        assert np.array_equal(sel.cls_thresh, g[f'sel/c{C}/thresh'][k]), k
        assert lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy(), g[f'sel/c{C}/labels'][k]), k


def test_generate_pseudo_writes_the_reference_files(gold, tmp_path):
    from regda_amd.utils.tools import generate_pseudo
    g = gold('iast.npz')
    C = 6
    probs, names = g[f'sel/c{C}/probs'], g[f'sel/c{C}/names']

    class Model:
        calls, mode = 0, None

        def eval(self):
            self.mode = 'eval'

        def __call__(self, image):
            assert image.is_cuda and self.mode == 'eval'
            self.calls += 1
            out = torch.from_numpy(probs[self.calls - 1]).cuda()
            return (out, None) if self.calls == 2 else out       # a tuple output: its first element

    loader = [(torch.zeros(2, 3, *probs.shape[-2:]), {'fname': list(names[k])}) for k in range(3)]
    written = []
    out_dir = generate_pseudo(Model(), loader, str(tmp_path), n_class=C, writer=lambda path, arr: written.append((path, arr)),
                              pseudo_dict=dict(pl_alpha=float(g['sel/alpha']), pl_beta=float(g['sel/beta']),
                                               pl_gamma=float(g['sel/gamma'])))
    assert out_dir == str(tmp_path / 'pred') and (tmp_path / 'pred').is_dir()
    assert [p for p, _ in written] == [str(tmp_path / 'pred' / f) for f in names.reshape(-1)]
    want = g[f'sel/c{C}/labels'].reshape(-1, *probs.shape[-2:])
    for (_, arr), ref in zip(written, want):
        assert isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and np.array_equal(arr, ref)


# ------------------------------------------------------------------------------------------------- the step
def _shallow():
    from test_losses_gpu import _shallow as shallow
    rt, sd, b, protos, ones, model = shallow()
    return {k: v.cuda() for k, v in b.items()}, protos, ones, model


def _args(g):
    return g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t']


def test_step_with_weights_zero_is_the_step_without_them():
    """ent_weight = kld_weight = 0: the same launches (the rows of a recorded plan) and the same bits."""
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    outs = []
    for kw in ({}, dict(ent_weight=0.0, kld_weight=0.0)):
        m = model()
        st = SSLStep(m, protos, **kw)
        o1 = [x.clone() for x in st.step(*_args(g), 1e-3)]
        stats = st.record_plan(*_args(g))
        outs.append((o1, [x.clone() for x in st._out], m.flat_p.clone(), stats))
        assert st.loss_ent is None and st.loss_kld is None
    (a1, a2, pa, sa), (b1, b2, pb, sb) = outs
    assert sa == sb
    for x, y in zip(a1 + a2 + [pa], b1 + b2 + [pb]):
        assert torch.equal(x, y)


@pytest.mark.parametrize('loss_t', ('none', 'uvem', 'gdp'))
def test_step_terms_and_their_gradient(loss_t):
    """loss_ent / loss_kld of the step against the restatement on the step's own target logits and final pseudo labels;
    the logit gradient is the weights-0 step's plus the regulariser's own (one f32 add); the recorded plan gives the
    eager step's bits."""
    from regda_amd import ops
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    lam = (0.3, 0.1)
    steps = {}
    for on in (False, True):
        m = model()
        st = SSLStep(m, protos, loss_t=loss_t, **(dict(ent_weight=lam[0], kld_weight=lam[1]) if on else {}))
        st.keep_debug = True
        out = [x.clone() for x in st.step(*_args(g), 1e-3)]
        steps[on] = (st, m, out, {k: v.clone() for k, v in st.debug.items() if k in ('t1', 't2', 'g1_t', 'g2_t')},
                     st.last_hard.clone())
    (st0, m0, out0, d0, hard0), (st1, m1, out1, d1, hard1) = steps[False], steps[True]
    assert torch.equal(d0['t1'], d1['t1']) and torch.equal(d0['t2'], d1['t2']) and torch.equal(hard0, hard1)
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])      # the reported losses are the unregularised ones
    assert not torch.equal(out0[2], out1[2])                                    # the gradient norm is not
    n_ign = int((hard1 == -1).sum())
    assert 0 < n_ign < hard1.numel()
    we, wk = iast_ref.derived_weights(hard1.cpu(), -1, torch.float64)
    ent, kld, _ = iast_ref.reg([d1['t1'].cpu().double(), d1['t2'].cpu().double()], hard1.shape[-2:], we, wk, *lam, True)
    print(f'[step {loss_t}] ent {float(st1.loss_ent):.9g} (restatement {float(ent):.9g}) kld {float(st1.loss_kld):.9g} '
          f'(restatement {float(kld):.9g}); {n_ign} of {hard1.numel()} pixels ignored')
    assert float(st1.loss_ent) == pytest.approx(float(ent), rel=1e-5)
    assert float(st1.loss_kld) == pytest.approx(float(kld), rel=1e-5)
    reg, r1, r2 = ops.upsample_reg(d1['t1'], d1['t2'], hard1, lambda_ent=lam[0], lambda_kld=lam[1], empty_is_zero=True)
    assert torch.equal(reg[0], st1.loss_ent) and torch.equal(reg[1], st1.loss_kld)
    assert r1.abs().sum() > 0 and torch.equal(d1['g1_t'], d0['g1_t'] + r1) and torch.equal(d1['g2_t'], d0['g2_t'] + r2)
    # step 2 eagerly and as the recording of a plan, then a replay against a third eager step
    m2 = model()
    st2 = SSLStep(m2, protos, loss_t=loss_t, ent_weight=lam[0], kld_weight=lam[1])
    st2.keep_debug = True
    st2.step(*_args(g), 1e-3)
    st1.keep_debug = st2.keep_debug = False
    eager = [[x.clone() for x in st1.step(*_args(g), 1e-3)] + [st1.loss_ent.clone(), st1.loss_kld.clone()] for _ in range(2)]
    st2.record_plan(*_args(g), lr=1e-3)
    planned = [[x.clone() for x in st2._out] + [st2.loss_ent.clone(), st2.loss_kld.clone()]]
    planned.append([x.clone() for x in st2.step(*_args(g), 1e-3)] + [st2.loss_ent.clone(), st2.loss_kld.clone()])
    for e, p in zip(eager, planned):
        for x, y in zip(e, p):
            assert torch.equal(x, y)
    assert torch.equal(m1.flat_p, m2.flat_p)
    assert not torch.equal(eager[0][3], eager[1][3])        # the terms move from step to step


def test_captured_graph_gives_the_eager_bits():
    from regda_amd.ssl import SSLStep
    g, protos, ones, model = _shallow()
    runs = []
    for captured in (False, True):
        m = model()
        m.set_drop_masks(ones.cuda(), ones.cuda())          # (device masks: nothing is copied from the host in capture)
        st = SSLStep(m, protos, loss_t='focal', ent_weight=0.3, kld_weight=0.1)
        st.step(*_args(g), 1e-3)
        if captured:
            st.capture(*_args(g))
        out = [x.clone() for x in st.step(*_args(g), 1e-3)] + [st.loss_ent.clone(), st.loss_kld.clone()]
        torch.cuda.synchronize()
        runs.append(out + [m.flat_p.clone()])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert float(runs[0][3]) > 0 and float(runs[0][4]) > 0
