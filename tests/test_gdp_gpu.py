"""GPU: the fused GDPLoss (rgda_upsample_gdp) and the prototype pixel weight (rgda_proto_pixel_weight) against the
reference's own classes (tests/golden/gdp.npz), against the CPU restatement (tests/gdp_ref.py) at edge shapes,
bit-identical repeats, and SSLStep(loss_t='gdp') against CPU steps that use the restatement in place of the oracle's
cross-entropy (oracle.labelpath.loss_calc / label_refine, monkeypatched as tests/test_losses_gpu.py does)."""
import numpy as np
import pytest
import torch

import gdp_ref
import loss_ref
from oracle import labelpath as olp
from test_gdp_cpu import CASES, case

pytestmark = pytest.mark.gpu


def _gdp(C, cb, pr, mom, balancer=None):
    from regda_amd.gast.balance import GDPLoss
    return GDPLoss(bins=30, momentum=mom, class_num=C, ignore_label=-1, class_balance=cb, prototype_refine=pr, temp=0.5,
                   class_balancer=balancer)


@pytest.mark.parametrize('name', sorted(CASES))
def test_fused_gdp_matches_the_reference_goldens(gold, name):
    """Every golden case through GDPLoss + loss_calc, with the tolerances tests/test_losses_gpu.py uses for GHM on its
    goldens: loss rel 2e-6, gradients rtol 2e-4 / atol 1e-8, acc_sum and bins_weight rtol 1e-6."""
    from regda_amd.utils.tools import loss_calc
    C, cb, pr, mom, calls, single = CASES[name]
    c = case(gold('gdp.npz'), name)
    fn = _gdp(C, cb, pr, mom)
    lab = torch.from_numpy(c['lab'].astype(np.int64)).cuda()
    if pr:
        fn.set_prototype_weight_4pixel(torch.from_numpy(c['pw']).cuda())
    for k in range(calls):
        sfx = '' if k == 0 else str(k)
        q1 = torch.from_numpy(c['p1']).cuda().requires_grad_(True)
        q2 = torch.from_numpy(c['p2']).cuda().requires_grad_(True)
        loss = loss_calc(q1, lab, fn, multi=False) if single else loss_calc([q1, q2], lab, fn, multi=True)
        loss.backward()
        ref = float(c['loss' + sfx])
        print(f'[{name}{sfx}] loss {float(loss.detach()):.9g} (reference {ref:.9g})')
        assert float(loss.detach()) == pytest.approx(ref, rel=2e-6, abs=0 if ref else 1e-12)
        np.testing.assert_allclose(q1.grad.cpu().numpy(), c['g1' + sfx], rtol=2e-4, atol=1e-8)
        if not single:
            np.testing.assert_allclose(q2.grad.cpu().numpy(), c['g2' + sfx], rtol=2e-4, atol=1e-8)
        np.testing.assert_allclose(fn.acc_sum.cpu().numpy(), c['acc' + sfx], rtol=1e-6)
        np.testing.assert_allclose(fn.bins_weight.cpu().numpy(), c['bw' + sfx], rtol=1e-6)
        if cb:
            np.testing.assert_allclose(fn.class_balancer.freq.cpu().numpy(), c['freq' + sfx], rtol=1e-6)
    if name == 'ignored':        # the reference's arithmetic: 0 / 1e-7 = 0, no gradient
        assert float(loss) == 0.0 and not q1.grad.any() and not q2.grad.any()
    dist, bw, report = fn.get_g_distribution()
    assert dist.shape == (30,) and bw is fn.bins_weight and report.startswith('class frequency: ')


# ------------------------------------------------------------------------------------------------- edge shapes
SHAPES = [(2, 6, 5, 7, 37, 300, 5), (1, 16, 8, 8, 128, 128, 6), (2, 7, 3, 20, 48, 516, 7)]
_EDGE = {}


def near_edges(p1, p2, lab, eps_floor=1e-5):
    """tests/test_losses_gpu.ignore_near_boundary('ghm', ...) for a label map of any aspect (that function upsamples to a
    square of the label's width): the pixels of either head whose |p_y - 1| lies within eps of a bin edge become ignored
    until none is left; eps = max(1e-5, 3 x the f32 rounding error of |p_y - 1| against float64)."""
    size = tuple(lab.shape[-2:])
    noise = 0.0
    for p in (p1, p2):
        v32, v64 = loss_ref.ghm_g(loss_ref.up(p, size), lab), loss_ref.ghm_g(loss_ref.up(p.double(), size), lab)
        noise = max(noise, float((v32.double() - v64).abs().max()))
    eps = max(eps_floor, 3 * noise)
    n = 0
    for _ in range(20):
        near = torch.zeros(lab.numel(), dtype=torch.bool)
        for p in (p1, p2):
            near |= loss_ref.near_boundary('ghm', loss_ref.up(p, size), lab, eps=eps)
        near &= lab.reshape(-1) != -1
        if not near.any():
            return lab, eps, n
        n += int(near.sum())
        lab = torch.where(near.reshape(lab.shape), torch.full_like(lab, -1), lab)
    raise AssertionError('pixels near a bin edge remain')


def edge_inputs(shape):
    """Inputs of one edge shape and the restatement's results for every variant, computed once per session."""
    if shape in _EDGE:
        return _EDGE[shape]
    from test_losses_gpu import ignore_near_boundary
    b, C, h, w, H, W, seed = shape
    g = torch.Generator().manual_seed(seed)
    p1, p2 = torch.randn(b, C, h, w, generator=g) * 2, torch.randn(b, C, h, w, generator=g) * 2
    lab0 = torch.randint(0, C, (b, H, W), generator=g)
    lab0 = torch.where(torch.rand(b, H, W, generator=g) < 0.1, torch.full_like(lab0, -1), lab0)
    pw = torch.rand(b * H * W, generator=g)
    f0 = torch.softmax(torch.randn(C, generator=g), 0)
    lab, eps, n = near_edges(p1, p2, lab0)
    if H == W:      # the square shape goes through that file's own function: the same pixels, the same eps
        lab_sq, eps_sq, n_sq = ignore_near_boundary('ghm', p1, p2, lab0, None)
        assert torch.equal(lab_sq, lab) and eps_sq == eps and n_sq == n
    print(f'[gdp {shape}] eps {eps:.1e}: {n} of {lab.numel()} pixels ignored')
    assert n < 0.002 * lab.numel()
    refs = {}
    for variant in ('plain', 'both', 'single', 'twice'):
        st = gdp_ref.GdpState(0.99)
        bal = gdp_ref.BalanceState(C, -1, 0.99, 0.5, f0) if variant in ('both', 'twice') else None
        out = []
        for _ in range(2 if variant == 'twice' else 1):
            r1, r2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
            ref = gdp_ref.loss_calc(r1 if variant == 'single' else [r1, r2], lab, st, -1,
                                    pw if variant in ('both', 'twice') else None, bal)
            ref.backward()
            out.append((ref.detach(), r1.grad, r2.grad, st.acc_sum.clone(), st.bins_weight.clone(),
                        None if bal is None else bal.freq.clone()))
        refs[variant] = out
    _EDGE[shape] = dict(p1=p1, p2=p2, lab=lab, pw=pw, f0=f0, refs=refs)
    return _EDGE[shape]


def run_variant(d, C, variant):
    """-> [(loss, g1, g2, acc_sum, bins_weight, freq) per call] of the fused loss, on the CPU"""
    from regda_amd.gast.balance import ClassBalance
    from regda_amd.utils.tools import loss_calc
    extra = variant in ('both', 'twice')
    bal = None
    if extra:
        bal = ClassBalance(C, -1, 0.99, 0.5)
        bal.freq = d['f0'].cuda()
    fn = _gdp(C, extra, extra, 0.99, bal)
    if extra:
        fn.set_prototype_weight_4pixel(d['pw'].cuda())
    lab = d['lab'].cuda()
    out = []
    for _ in range(2 if variant == 'twice' else 1):
        q1, q2 = d['p1'].cuda().requires_grad_(True), d['p2'].cuda().requires_grad_(True)
        loss = loss_calc(q1, lab, fn, multi=False) if variant == 'single' else loss_calc([q1, q2], lab, fn, multi=True)
        loss.backward()
        out.append((loss.detach().cpu(), q1.grad.cpu(), None if variant == 'single' else q2.grad.cpu(),
                    fn.acc_sum.cpu().clone(), fn.bins_weight.cpu().clone(), None if bal is None else bal.freq.cpu().clone()))
    return out


@pytest.mark.parametrize('variant', ['plain', 'both', 'single', 'twice'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s[:6])))
def test_fused_gdp_edge_shapes_against_the_restatement(shape, variant):
    """Rows longer than one 256-thread sweep, W no multiple of 4, 16 classes, wide low-resolution rows: loss, every logit
    gradient, acc_sum, bins_weight and the balancer against tests/gdp_ref.py, with the tolerances of
    tests/test_losses_gpu.py::test_fused_losses_full_size_against_the_restatement.  variant: without / with pixel and
    class weights, one prediction (heads=1), two consecutive calls."""
    d = edge_inputs(shape)
    for k, (got, want) in enumerate(zip(run_variant(d, shape[1], variant), d['refs'][variant])):
        loss, g1, g2, acc, bw, freq = got
        rloss, r1, r2, racc, rbw, rfreq = want
        print(f'[gdp {shape} {variant} call {k}] loss {float(loss):.9g} (restatement {float(rloss):.9g})')
        assert float(loss) == pytest.approx(float(rloss), rel=1e-5)
        for a, r in ((g1, r1), (g2, r2)):
            if a is not None:
                np.testing.assert_allclose(a.numpy(), r.numpy(), rtol=1e-3, atol=1e-4 * float(r.abs().max()))
        np.testing.assert_allclose(acc.numpy(), racc.numpy(), rtol=1e-5)
        np.testing.assert_allclose(bw.numpy(), rbw.numpy(), rtol=1e-5)
        if freq is not None:
            np.testing.assert_allclose(freq.numpy(), rfreq.numpy(), rtol=1e-6)


@pytest.mark.parametrize('extra', [False, True])
def test_fused_gdp_is_bit_identical_from_run_to_run(extra):
    from regda_amd import ops
    d = edge_inputs(SHAPES[2])
    p1, p2, lab = d['p1'].cuda(), d['p2'].cuda(), d['lab'].cuda()
    pw = d['pw'].cuda() if extra else None
    cw = torch.rand(2, SHAPES[2][1], generator=torch.Generator().manual_seed(1)).cuda() if extra else None
    outs = []
    for _ in range(2):
        acc, bw = torch.zeros(30, device='cuda'), torch.zeros(30, device='cuda')
        res = ()
        for _call in range(2):          # two calls: the state of the first feeds the second
            res += ops.upsample_gdp(p1, p2, lab, acc, bw, pixel_weight=pw, class_weight=cw, momentum=0.99)
            res += (acc.clone(), bw.clone())
        outs.append(res)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[0][0]) > 0 and outs[0][1].abs().sum() > 0


# ------------------------------------------------------------------------------------------------- prototype weights
PW_SHAPES = [(2, 6, 64, 5, 7, 37, 300), (1, 16, 2048, 4, 4, 64, 64)]


def pw_inputs(shape):
    b, C, K, h, w, H, W = shape
    g = torch.Generator().manual_seed(40 + C)
    feat, protos = torch.randn(b, K, h, w, generator=g), torch.randn(C, K, generator=g)
    lab = torch.randint(0, C, (b, H, W), generator=g)
    lab = torch.where(torch.rand(b, H, W, generator=g) < 0.15, torch.full_like(lab, -1), lab)
    return feat, protos, lab


@pytest.mark.parametrize('shape', PW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_proto_pixel_weight_against_the_restatement(shape):
    """Against the restatement in fp64; bound max(3 x |fp32 restatement - fp64 restatement|, 1e-4) (the floor: the
    project's bound for the refine goldens).  The similarity map label_refine leaves in its workspace gives the same bits."""
    from regda_amd import ops
    feat, protos, lab = pw_inputs(shape)
    b, C, K, h, w, H, W = shape
    r64 = gdp_ref.proto_weight(feat.double(), protos.double(), lab)
    r32 = gdp_ref.proto_weight(feat, protos, lab)
    bound = max(3 * float((r32.double() - r64).abs().max()), 1e-4)
    got = ops.proto_pixel_weight(feat.cuda(), protos.cuda(), lab.cuda())
    assert got.shape == (b * H * W,) and got.dtype == torch.float32
    err = float((got.cpu().double() - r64).abs().max())
    print(f'[proto_pixel_weight {shape}] max err {err:.2e} (bound {bound:.2e})')
    assert err <= bound
    ign = (lab == -1).reshape(-1)
    assert not got.cpu()[ign].any() and float(got.max()) <= 1.0 and float(got.cpu()[~ign].min()) > 0
    # sim= from label_refine's workspace: bit-identical to the call that computes its own
    g = torch.Generator().manual_seed(3)
    p1, p2 = torch.randn(b, C, h, w, generator=g).cuda(), torch.randn(b, C, h, w, generator=g).cuda()
    soft = torch.softmax(torch.randn(b, C, H, W, generator=g), 1).cuda()
    _, _, sim = ops.label_refine(feat.cuda(), protos.cuda(), p1, p2, soft, 2.0, return_ws=True, return_sim=True)
    assert sim.shape == (b, C, h, w)
    np.testing.assert_allclose(sim.cpu().numpy(), gdp_ref.pearson_sim(feat, protos).numpy(), rtol=2e-3)
    again = ops.proto_pixel_weight(None, None, lab.cuda(), sim=sim)
    assert torch.equal(again, got)
    assert torch.equal(ops.proto_pixel_weight(feat.cuda(), protos.cuda(), lab.cuda()), got)      # and from run to run


@pytest.mark.parametrize('C', [6, 7])
def test_aligner_prototype_weight_matches_the_reference_golden(gold, C):
    from regda_amd.gast.alignment import Aligner
    g = gold('gdp.npz')
    al = Aligner(None, feat_channels=64, class_num=C, ignore_label=-1)
    al.prototypes = torch.from_numpy(g[f'c{C}/protos']).cuda()
    lab = torch.from_numpy(g[f'c{C}/lab'].astype(np.int64)).cuda()
    w = al.get_prototype_weight_4pixel(torch.from_numpy(g[f'c{C}/feat']).cuda(), lab, temp=2.0)
    assert w.shape == (lab.numel(),) and not w.requires_grad
    np.testing.assert_allclose(w.cpu().numpy(), g[f'c{C}/pw'], rtol=0, atol=1e-4)
    # (b, 1, H, W) labels, as the reference's _index2onehot accepts
    assert torch.equal(al.get_prototype_weight_4pixel(torch.from_numpy(g[f'c{C}/feat']).cuda(), lab[:, None]), w)


# ------------------------------------------------------------------------------------------------- steps
def _patch_oracle(monkeypatch, state, proto, balancer_t):
    """oracle.labelpath.loss_calc -> source: the oracle's own CE; target: the restated GDPLoss, with the prototype
    weights built from the features and prototypes the step's label_refine was given (recorded here)."""
    seen = {'n': 0}
    refine, ce = olp.label_refine, olp.loss_calc

    def label_refine(feat_t, prototypes, *a, **k):
        seen['feat_t'], seen['protos'] = feat_t.detach().clone(), prototypes.detach().clone()
        return refine(feat_t, prototypes, *a, **k)

    def loss_calc(preds, label, ignore_label=-1, balancer=None):
        is_t = seen['n'] % 2 == 1
        seen['n'] += 1
        if not is_t:
            return ce(preds, label, ignore_label, balancer)
        pw = gdp_ref.proto_weight(seen['feat_t'], seen['protos'], label, ignore_label) if proto else None
        return gdp_ref.loss_calc(list(preds), label, state, ignore_label, pw, balancer_t)
    monkeypatch.setattr(olp, 'loss_calc', loss_calc)
    monkeypatch.setattr(olp, 'label_refine', label_refine)


def _cpu_refs(monkeypatch, fx, proto, f0t, emulate_bf16):
    from oracle.step import CpuStep
    rt, sd, b, protos, ones, _ = fx
    state = gdp_ref.GdpState(0.99)
    bal = None
    if f0t is not None:
        bal = olp.ClassBalanceState(6, -1, 0.5, 0.5)
        bal.freq = f0t.clone()
    _patch_oracle(monkeypatch, state, proto, bal)
    cpu = CpuStep(sd, protos, resnet_type=rt, lr=1e-3, emulate_bf16=emulate_bf16)
    refs = [cpu.step(b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'], (ones, ones), (ones, ones))
            for _ in range(2)]
    monkeypatch.undo()
    return refs, state, bal


@pytest.mark.parametrize('proto,cb', [(True, False), (False, False), (True, True)])
def test_ssl_step_with_gdp_matches_the_cpu_step(monkeypatch, proto, cb):
    """SSLStep(loss_t='gdp') for two steps, eagerly and as a recorded plan, against oracle.step.CpuStep with the restated
    GDPLoss: both losses, the gradient norm, acc_sum and the balancer's frequencies.  Bounds: tests/test_losses_gpu.py's
    _bound rule (three times the bf16-emulating CPU step's distance from the fp32 CPU step, or its floor).  The run with
    overlap_wgrad=False (one stream) matches the two-stream run bit for bit: the prototype weights come from the
    prototypes as label_refine read them, whichever stream rewrites them afterwards."""
    from regda_amd.gast.balance import ClassBalance
    from regda_amd.ssl import SSLStep
    from test_losses_gpu import _bound, _shallow
    from test_ssl_step_gpu import tol, tol_gn
    FB = 'shallow_step_class_balancing'
    fx = _shallow()
    rt, sd, b, protos, ones, model = fx
    f0t = torch.tensor([0.05, 0.05, 0.1, 0.1, 0.2, 0.5]) if cb else None
    refs, state, bal = _cpu_refs(monkeypatch, fx, proto, f0t, False)
    emus, state_e, _ = _cpu_refs(monkeypatch, fx, proto, f0t, True)
    g = {k: v.cuda() for k, v in b.items()}
    args = (g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'])
    vals = lambda o: [float(x.item()) for x in o]
    finals = {}
    for mode in ('eager', 'plan') + (('one_stream',) if proto and not cb else ()):
        bt = None
        if cb:
            bt = ClassBalance(6, -1, 0.5, 0.5)
            bt.freq = f0t.cuda()
        st = SSLStep(model(), protos, loss_t='gdp', gdp_prototype=proto, gdp_class_balance=cb, class_balancer_t=bt,
                     overlap_wgrad=mode != 'one_stream')
        assert (st.loss_fn_t.class_balancer is bt) if cb else (st.loss_fn_t.class_balancer is None)
        outs = [vals(st.step(*args, 1e-3))]
        acc1 = st.loss_fn_t.acc_sum.clone()
        if mode == 'plan':
            st.record_plan(*args)
            outs.append(vals(st._out))
        else:
            outs.append(vals(st.step(*args, 1e-3)))
        assert (st.last_proto_weight is not None) == proto
        finals[mode] = (outs, st.loss_fn_t.acc_sum.clone(), st.loss_fn_t.bins_weight.clone(),
                        None if not proto else st.last_proto_weight.clone())
        for (ls, lt, gn), ref, emu in zip(outs, refs, emus):
            b_s = _bound('loss_source', ref, emu, tol(FB, 'loss_source'))
            b_t = _bound('loss_target', ref, emu, tol(FB, 'loss_target'))
            b_g = _bound('grad_norm', ref, emu, tol_gn(FB))
            print(f'[gdp proto={proto} cb={cb} {mode}] rel dev: source {abs(ls / ref["loss_source"] - 1):.2e} (bound '
                  f'{b_s:.1e}), target {abs(lt / ref["loss_target"] - 1):.2e} (bound {b_t:.1e}), |g| '
                  f'{abs(gn ** 0.5 / ref["grad_norm"] - 1):.2e} (bound {b_g:.1e})')
            assert ls == pytest.approx(ref['loss_source'], rel=b_s), mode
            assert lt == pytest.approx(ref['loss_target'], rel=b_t, abs=tol(FB, 'loss_target_abs')), mode
            assert gn ** 0.5 == pytest.approx(ref['grad_norm'], rel=b_g), mode
        # acc_sum after four head calls: the histogram of |p_y - 1| of the bf16 network; per bin three times the
        # bf16-emulating step's distance, floored as the GHM step test floors it (15 % + 0.05)
        got, want = st.loss_fn_t.acc_sum.cpu().numpy(), state.acc_sum.numpy()
        assert not torch.equal(st.loss_fn_t.acc_sum, acc1)          # the state advanced in the second step / the recording
        assert got.sum() == pytest.approx(float(want.sum()), rel=1e-2)
        bound = np.maximum(3 * np.abs(state_e.acc_sum.numpy() - want), 0.15 * np.abs(want) + 0.05)
        print(f'[gdp proto={proto} cb={cb} {mode}] acc_sum max dev / bound {np.max(np.abs(got - want) / bound):.2f}')
        assert (np.abs(got - want) <= bound).all()
        if cb:                      # four EMA updates (two heads x two steps) on the pseudo labels
            torch.testing.assert_close(bt.freq.cpu(), bal.freq, rtol=0, atol=tol(FB, 'freq_t_abs', floor=2e-4))
        if mode == 'plan':          # a replay advances the state again
            acc2 = st.loss_fn_t.acc_sum.clone()
            st.step(*args, 1e-3)
            assert not torch.equal(st.loss_fn_t.acc_sum, acc2)
    if 'one_stream' in finals:      # the ordering check
        (o2, acc2, bw2, pw2), (o1, acc1_, bw1, pw1) = finals['eager'], finals['one_stream']
        assert o1 == o2 and torch.equal(acc1_, acc2) and torch.equal(bw1, bw2) and torch.equal(pw1, pw2)


def test_ssl_step_with_gdp_without_label_refine_keeps_the_prototype_order():
    """refine_label=False: the prototype weights read the prototypes themselves, so the side stream's update_prototype is
    released only behind them -- one stream and two streams give the same bits, and a captured step replays them."""
    from regda_amd.ssl import SSLStep
    from test_losses_gpu import _shallow
    rt, sd, b, protos, ones, model = _shallow()
    g = {k: v.cuda() for k, v in b.items()}
    args = (g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'])
    runs = []
    for overlap in (True, False):
        st = SSLStep(model(), protos, loss_t='gdp', refine_label=False, overlap_wgrad=overlap)
        outs = [[float(x.item()) for x in st.step(*args, 1e-3)] for _ in range(2)]
        runs.append((outs, st.loss_fn_t.acc_sum.clone(), st.last_proto_weight.clone(), st.prototypes.clone()))
    for a, b_ in zip(*runs):
        assert a == b_ if isinstance(a, list) else torch.equal(a, b_)
    assert float(runs[0][2].max()) > 0


def test_ssl_step_with_gdp_captured_replay_matches_eager():
    """No host-side balancer: the whole step can be captured.  Step 1 eager, then step 2 as a graph replay, against the
    same two steps eager: losses, gradient norm, acc_sum and bins_weight agree, and a further replay advances acc_sum."""
    from regda_amd.ssl import SSLStep
    from test_losses_gpu import _shallow
    rt, sd, b, protos, ones, model = _shallow()
    g = {k: v.cuda() for k, v in b.items()}
    args = (g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'])
    runs = []
    for captured in (False, True):
        m = model()
        m.set_drop_masks(ones.cuda(), ones.cuda())          # (device masks: nothing is copied from the host in capture)
        st = SSLStep(m, protos, loss_t='gdp')
        st.step(*args, 1e-3)
        if captured:
            st.capture(*args)
        out = [float(x.item()) for x in st.step(*args, 1e-3)]
        runs.append((out, st.loss_fn_t.acc_sum.clone(), st.loss_fn_t.bins_weight.clone(), st))
    (eager, acc_e, bw_e, _), (graph, acc_g, bw_g, st) = runs
    for a, b_ in zip(graph, eager):
        assert a == pytest.approx(b_, rel=1e-5)
    torch.testing.assert_close(acc_g, acc_e, rtol=1e-5, atol=0)
    torch.testing.assert_close(bw_g, bw_e, rtol=1e-5, atol=1e-7)
    st.step(*args, 1e-3)
    assert not torch.equal(st.loss_fn_t.acc_sum, acc_g)
