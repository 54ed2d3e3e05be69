"""GPU: the fused --ls / --lt losses (rgda_upsample_loss: OhemCrossEntropy, FocalLoss, GHMLoss, UPSLoss, UVEMLoss)
against the reference's own classes (tests/golden/losses.npz), against the CPU restatement (tests/loss_ref.py) at the
production map sizes, bit-identical repeats, and the steps built with loss_s / loss_t against CPU steps that use the
restatement in place of the oracle's cross-entropy (oracle.labelpath.loss_calc, monkeypatched)."""
import numpy as np
import pytest
import torch

import loss_ref
from oracle import labelpath as olp

pytestmark = pytest.mark.gpu

F0 = torch.tensor([0.4, 0.25, 0.1, 0.1, 0.1, 0.05])
CASES = ['ohem', 'ohem_topk', 'ohem_bal', 'ohem_ignored', 'focal', 'ghm', 'ups', 'ups_bal', 'uvem', 'uvem_bal',
         'uvem_zeros', 'ups_zeros', 'uvem_onehot']
KINDS = ['ohem', 'focal', 'ghm', 'ups', 'uvem']
# stage-1 / stage-2 step parity: the bounds of the existing SourceStep / AlignStep tests (tests/test_coral_gpu.py); the
# SSL step test derives its bounds per configuration (_bound)
STEP_LOSS_REL, STEP_GN_REL = 2e-2, 6e-2


def case(g, name):
    return {k.split('/', 1)[1]: g[k] for k in g.files if k.startswith(name + '/')}


def fused(kind, bal=None, ghm_momentum=0.99):
    from regda_amd.gast import balance as B
    if kind == 'ohem':
        return B.OhemCrossEntropy(ignore_label=-1, class_balancer=bal)
    if kind == 'focal':
        return B.FocalLoss(gamma=2.0, reduction='mean', ignore_label=-1)
    if kind == 'ghm':
        return B.GHMLoss(bins=30, momentum=ghm_momentum, ignore_label=-1)
    if kind == 'ups':
        return B.UPSLoss(threshold=0.7, class_balancer=bal, class_num=6, ignore_label=-1)
    return B.UVEMLoss(m=0.2, threshold=0.7, gamma=4.0, class_balancer=bal, class_num=6, ignore_label=-1)


def run_fused(fn, kind, p1, p2, lab, soft):
    from regda_amd.gast.balance import loss_calc_uvem
    from regda_amd.utils.tools import loss_calc
    q1, q2 = p1.cuda().requires_grad_(True), p2.cuda().requires_grad_(True)
    if kind in ('ups', 'uvem'):
        loss = loss_calc_uvem([q1, q2], lab.cuda(), soft.cuda(), fn, multi=True)
    else:
        loss = loss_calc([q1, q2], lab.cuda(), fn, multi=True)
    loss.backward()
    return loss.detach().cpu(), q1.grad.cpu(), q2.grad.cpu()


@pytest.mark.parametrize('name', CASES)
def test_fused_losses_match_the_reference_goldens(gold, name):
    from regda_amd.gast.balance import ClassBalance
    c = case(gold('losses.npz'), name)
    kind = name.split('_')[0]
    bal = None
    if name.endswith('_bal'):
        bal = ClassBalance(6, -1, 0.9, 2.0)
        bal.freq = F0.cuda()
    fn = fused(kind, bal)
    p1, p2 = torch.from_numpy(c['p1']), torch.from_numpy(c['p2'])
    lab = torch.from_numpy(c['lab'].astype(np.int64))
    soft = torch.from_numpy(c['soft']) if 'soft' in c else None
    for k in range(2 if kind == 'ghm' else 1):
        sfx = '' if k == 0 else str(k)
        loss, g1, g2 = run_fused(fn, kind, p1, p2, lab, soft)
        ref = float(c['loss' + sfx])
        if np.isnan(ref):
            assert torch.isnan(loss)
        else:
            assert float(loss) == pytest.approx(ref, rel=2e-6)
        # (a one-hot soft label divides by 1e-7: gradients of order 1e7, f32 sums of such terms agree to ~1e-3)
        rtol = 1e-3 if name == 'uvem_onehot' else 2e-4
        np.testing.assert_allclose(g1.numpy(), c['g1' + sfx], rtol=rtol, atol=1e-8)
        np.testing.assert_allclose(g2.numpy(), c['g2' + sfx], rtol=rtol, atol=1e-8)
        if kind == 'ghm':
            np.testing.assert_allclose(fn.acc_sum.cpu().numpy(), c['acc' + sfx], rtol=1e-6)
    if bal is not None:
        np.testing.assert_allclose(bal.freq.cpu().numpy(), c['freq'], rtol=1e-6)
    if name == 'ohem_ignored':
        assert not g1.any() and not g2.any()


def full_size_inputs(seed, confident=False):
    g = torch.Generator().manual_seed(seed)
    b, H = 4, 512
    p1 = torch.randn(b, 6, 32, 32, generator=g) * 2
    p2 = torch.randn(b, 6, 32, 32, generator=g) * 2
    lab = torch.randint(0, 6, (b, H, H), generator=g)
    if confident:
        # OHEM's top-k branch with a gap at the k-th place: labels = the prediction; pixels whose CE lies between 0.01
        # and 0.3 in either head are ignored; then exactly n_min = #valid / 5 pixels get a large CE (those above 0.3,
        # topped up by relabelled confident ones), and only some of them exceed -log(0.7)
        base = torch.randn(b, 6, 32, 32, generator=g) * 24
        p1 = base + torch.randn(b, 6, 32, 32, generator=g) * 0.2
        p2 = base + torch.randn(b, 6, 32, 32, generator=g) * 0.2
        lab = loss_ref.up(base, (H, H)).argmax(1)
        v = torch.stack([loss_ref._ce(loss_ref.up(p, (H, H)), lab, -1) for p in (p1, p2)])
        low, high = v.amax(0) < 0.01, v.amin(0) > 0.3
        keep = (low | high) & (torch.rand(b * H * H, generator=g) >= 0.15)
        n_min = int(keep.sum()) // 5
        cand = torch.nonzero(low & keep)[:, 0]
        n_flip = n_min - int((high & keep).sum())
        assert n_flip > 0
        flip = cand[torch.randperm(cand.numel(), generator=g)[:n_flip]]
        lab = lab.reshape(-1)
        lab[flip] = (lab[flip] + 1) % 6
        lab = torch.where(keep, lab, torch.full_like(lab, -1)).reshape(b, H, H)
        soft = torch.softmax(torch.randn(b, 6, H, H, generator=g) * 3, 1)
        return p1, p2, lab, soft
    soft = torch.softmax(torch.randn(b, 6, H, H, generator=g) * 3, 1)
    return p1, p2, lab, soft


def decision_values(kind, p_full, label, soft):
    """the per-pixel value a loss decides on (OHEM: the CE, GHM: |p_y - 1|, UPS / UVEM: u), at the precision of p_full"""
    if kind == 'ohem':
        return loss_ref._ce(p_full, label, -1).detach()
    if kind == 'ghm':
        return loss_ref.ghm_g(p_full, label)
    return loss_ref.entropy(soft.to(p_full.dtype))


def ignore_near_boundary(kind, p1, p2, lab, soft, confident=False):
    """-> (labels, eps, n): the pixels of either head whose decision value lies within eps of a boundary of the loss
    (tests/loss_ref.near_boundary) become ignored, on both sides of the comparison, until none is left.  eps is 1e-5,
    or three times the f32 rounding error of the decision value where that is larger (measured here on the CPU against
    float64: the OHEM logits carry ~2e-5 of interpolation error into the CE).  For the top-k branch the inputs are built
    with a gap at the k-th place (full_size_inputs), which is checked instead."""
    H = lab.shape[-1]
    noise = 0.0
    for p in (p1, p2):
        v32 = decision_values(kind, loss_ref.up(p, (H, H)), lab, soft)
        v64 = decision_values(kind, loss_ref.up(p.double(), (H, H)), lab, soft)
        ok = torch.isfinite(v32) & torch.isfinite(v64)
        if ok.any():
            noise = max(noise, float((v32.double() - v64)[ok].abs().max()))
    eps = max(1e-5, 3 * noise)
    if confident:
        # top-k branch: no pixel may be near the cut between the n_min-th and the next largest loss
        for p in (p1, p2):
            srt = torch.sort(decision_values(kind, loss_ref.up(p, (H, H)), lab, soft), descending=True).values
            n_min = int((lab != -1).sum()) // 5
            assert float(srt[n_min - 1] - srt[n_min]) > 2 * eps
        return lab, eps, 0
    n = 0
    for _ in range(20):
        near = torch.zeros(lab.numel(), dtype=torch.bool)
        for p in (p1, p2):
            near |= loss_ref.near_boundary(kind, loss_ref.up(p, (H, H)), lab, soft, eps=eps)
        near &= lab.reshape(-1) != -1
        if not near.any():
            return lab, eps, n
        n += int(near.sum())
        lab = torch.where(near.reshape(lab.shape), torch.full_like(lab, -1), lab)
    raise AssertionError('pixels near a decision boundary remain')


@pytest.mark.parametrize('kind,confident', [(k, False) for k in KINDS] + [('ohem', True)])
def test_fused_losses_full_size_against_the_restatement(kind, confident):
    """4 x 6 x 32 x 32 -> 512 x 512: loss, every logit gradient and GHM's state against tests/loss_ref.py.  Pixels
    whose decision value lies near a boundary of the loss are ignored on both sides (ignore_near_boundary)."""
    p1, p2, lab, soft = full_size_inputs(5, confident)
    lab, eps, n_ignored = ignore_near_boundary(kind, p1, p2, lab, soft, confident)
    print(f'[{kind}{" top-k" if confident else ""}] eps {eps:.1e}: {n_ignored} of {lab.numel()} pixels ignored')
    assert n_ignored < 0.002 * lab.numel()
    st = loss_ref.GhmState(0.99)
    fn = loss_ref.make_loss(kind, ghm_state=st)
    r1, r2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    ref = loss_ref.loss_calc([r1, r2], lab, fn, soft)
    ref.backward()
    if confident:
        for p in (p1, p2):
            v = loss_ref._ce(loss_ref.up(p, (512, 512)), lab, -1)
            assert int((v > loss_ref.OHEM_THRESH).sum()) < int((lab != -1).sum()) // 5
    ours = fused(kind)
    loss, g1, g2 = run_fused(ours, kind, p1, p2, lab, soft)
    assert float(loss) == pytest.approx(float(ref), rel=1e-5)
    for got, want in ((g1, r1.grad), (g2, r2.grad)):
        # rtol as tests/test_label_gpu.py::test_loss_full_size_vs_oracle (sums over ~1000 full-resolution pixels per
        # logit); the absolute floor: p - 1 of a confident pixel is exact to ~1 ulp of 1 in either implementation
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-3, atol=1e-4 * float(want.abs().max()))
    if kind == 'ghm':
        np.testing.assert_allclose(ours.acc_sum.cpu().numpy(), st.acc_sum.numpy(), rtol=1e-5)


def test_nan_and_one_hot_soft_label_cases():
    from regda_amd.gast import balance as B
    p1, p2, lab, soft = full_size_inputs(9)
    # every label ignored: OHEM's loss is NaN and its gradient exactly 0
    loss, g1, g2 = run_fused(B.OhemCrossEntropy(), 'ohem', p1, p2, torch.full_like(lab, -1), None)
    assert torch.isnan(loss) and not g1.any() and not g2.any()
    # a one-hot soft label: u = NaN everywhere, nothing counted: sum / 1e-7, with the UVEM weight at NaN
    hot = torch.nn.functional.one_hot(lab.clamp(min=0), 6).permute(0, 3, 1, 2).float()
    for kind in ('uvem', 'ups'):
        fn = loss_ref.make_loss(kind)
        ref = loss_ref.loss_calc([p1, p2], lab, fn, hot)
        loss, _, _ = run_fused(fused(kind), kind, p1, p2, lab, hot)
        assert float(ref) > 1e8 and float(loss) == pytest.approx(float(ref), rel=1e-5)
    w = loss_ref.uvem_weight(torch.tensor([float('nan')]), 0.2, 0.7, 4.0)
    assert float(w) == pytest.approx(0.9573, abs=1e-4)


@pytest.mark.parametrize('kind,confident', [(k, False) for k in KINDS] + [('ohem', True)])
def test_fused_losses_are_bit_identical_from_run_to_run(kind, confident):
    from regda_amd import ops
    p1, p2, lab, soft = (t.cuda() for t in full_size_inputs(3, confident))
    outs = []
    for _ in range(2):
        acc = torch.zeros(30, device='cuda')
        outs.append(ops.upsample_loss(kind, p1, p2, lab, soft=soft if kind in ('ups', 'uvem') else None,
                                      acc_sum=acc if kind == 'ghm' else None, thresh=loss_ref.OHEM_THRESH,
                                      momentum=0.99, gamma=2.0 if kind == 'focal' else 4.0) + (acc,))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_single_prediction_forward_is_one_call():
    """loss_fn(pred, label) on one prediction (loss_calc(multi=False)): one loss call, GHM's state updated once."""
    p1, _, lab0, soft = full_size_inputs(4)
    for kind in KINDS:
        lab, _, _ = ignore_near_boundary(kind, p1, p1, lab0, soft)
        st = loss_ref.GhmState(0.99)
        fn = loss_ref.make_loss(kind, ghm_state=st)
        r = p1.clone().requires_grad_(True)
        ref = fn(loss_ref.up(r, (512, 512)), lab, soft)
        ref.backward()
        ours = fused(kind)
        q = p1.cuda().requires_grad_(True)
        args = (soft.cuda(),) if kind in ('ups', 'uvem') else ()
        loss = ours(q, lab.cuda(), *args)
        loss.backward()
        assert float(loss) == pytest.approx(float(ref), rel=1e-5), kind
        np.testing.assert_allclose(q.grad.cpu().numpy(), r.grad.numpy(), rtol=1e-3, atol=1e-4 * float(r.grad.abs().max()))
        if kind == 'ghm':
            np.testing.assert_allclose(ours.acc_sum.cpu().numpy(), st.acc_sum.numpy(), rtol=1e-5)


# ------------------------------------------------------------------------------------------------- steps
def _patch_oracle(monkeypatch, kind_s, kind_t, ghm_state=None):
    """oracle.labelpath.loss_calc -> the restatement: calls alternate source / target within a CpuStep step (the
    CpuAlignStep makes source calls only: kind_t=None); ups / uvem read the refined soft label of the step."""
    seen = {'soft': None, 'n': 0}
    refine = olp.label_refine

    def label_refine(*a, **k):
        seen['soft'] = refine(*a, **k)
        return seen['soft']

    def loss_calc(preds, label, ignore_label=-1, balancer=None):
        is_t = kind_t is not None and seen['n'] % 2 == 1
        seen['n'] += 1
        kind = kind_t if is_t else kind_s
        fn = loss_ref.make_loss(kind, balancer=balancer, ghm_state=ghm_state)
        return loss_ref.loss_calc(preds, label, fn, seen['soft'] if is_t else None)
    monkeypatch.setattr(olp, 'loss_calc', loss_calc)
    monkeypatch.setattr(olp, 'label_refine', label_refine)


def _shallow():
    from oracle import model as omodel
    from regda_amd.synthetic import make_batch
    from test_ssl_step_gpu import build
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, 6, seed=6)
    b = make_batch(b=4, size=128, seed=11, device='cpu')
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(1))
    ones = torch.ones(4, 512)

    def model():
        m = build(rt)
        m.load_state_dict(sd, strict=True)
        m.set_drop_masks(ones, ones)
        return m
    return rt, sd, b, protos, ones, model


def _cpu_refs(monkeypatch, sd, protos, rt, b, ones, ks, kt, emulate_bf16, f0t=None):
    """two CpuStep iterations with the restated losses: (results, GHM state, target balancer)"""
    from oracle.step import CpuStep
    ghm = loss_ref.GhmState(0.99)
    bal = None
    if f0t is not None:
        bal = olp.ClassBalanceState(6, -1, 0.5, 0.5)
        bal.freq = f0t.clone()
    _patch_oracle(monkeypatch, ks, kt, ghm)
    cpu = CpuStep(sd, protos, resnet_type=rt, lr=1e-3, balancer_t=bal, emulate_bf16=emulate_bf16)
    refs = [cpu.step(b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'], (ones, ones), (ones, ones))
            for _ in range(2)]
    monkeypatch.undo()
    return refs, ghm, bal


def _bound(key, fp32, bf16, floor):
    """tolerance = max(3 N, floor) as in tests/test_ssl_step_gpu.py, N = |bf16-emulating CPU step - fp32 CPU step| of
    THIS loss configuration (relative), the floor the derived bound of the class-balancing step fixture"""
    return max(3 * abs(bf16[key] - fp32[key]) / abs(fp32[key]), floor)


@pytest.mark.parametrize('loss_t,loss_s,bct', [(k, 'CrossEntropy', False) for k in ('uvem', 'ups', 'ohem', 'focal', 'ghm')] +
                         [('uvem', 'CrossEntropy', True), ('none', 'OhemCrossEntropy', False)])
def test_ssl_step_with_loss_flags_matches_the_cpu_step(monkeypatch, loss_t, loss_s, bct):
    """SSLStep(loss_s=..., loss_t=...) for two steps, eagerly and as a recorded plan, against oracle.step.CpuStep with
    the restated losses: both losses and the gradient norm, GHM's state and (--bct) the target balancer's frequencies.
    Bounds: three rounding-noise units of each configuration, N = bf16-emulating CPU step against the fp32 CPU step,
    floored at the derived bounds of the class-balancing step fixture."""
    from regda_amd.gast.balance import ClassBalance
    from regda_amd.ssl import SSLStep
    from test_ssl_step_gpu import tol, tol_gn
    FB = 'shallow_step_class_balancing'
    rt, sd, b, protos, ones, model = _shallow()
    kt = {'none': 'ce', 'ours': 'uvem'}.get(loss_t, loss_t)
    ks = 'ce' if loss_s == 'CrossEntropy' else 'ohem'
    f0t = torch.tensor([0.05, 0.05, 0.1, 0.1, 0.2, 0.5]) if bct else None
    refs, ghm, bal = _cpu_refs(monkeypatch, sd, protos, rt, b, ones, ks, kt, False, f0t)
    emus, _, _ = _cpu_refs(monkeypatch, sd, protos, rt, b, ones, ks, kt, True, f0t)
    g = {k: v.cuda() for k, v in b.items()}
    for use_plan in (False, True):
        bt = None
        if bct:
            bt = ClassBalance(6, -1, 0.5, 0.5)
            bt.freq = f0t.cuda()
        st = SSLStep(model(), protos, loss_s=loss_s, loss_t=loss_t, class_balancer_t=bt)
        vals = lambda o: [float(x.item()) for x in o]
        outs = [vals(st.step(g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'], 1e-3))]
        if use_plan:
            st.record_plan(g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'])
            outs.append(vals(st._out))
        else:
            outs.append(vals(st.step(g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'], 1e-3)))
        for (ls, lt, gn), ref, emu in zip(outs, refs, emus):
            b_s = _bound('loss_source', ref, emu, tol(FB, 'loss_source'))
            b_t = _bound('loss_target', ref, emu, tol(FB, 'loss_target'))
            b_g = _bound('grad_norm', ref, emu, tol_gn(FB))
            print(f'[{loss_s} / {loss_t}{" bct" if bct else ""}{" plan" if use_plan else ""}] rel dev: source '
                  f'{abs(ls / ref["loss_source"] - 1):.2e} (bound {b_s:.1e}), target {abs(lt / ref["loss_target"] - 1):.2e} '
                  f'(bound {b_t:.1e}), |g| {abs(gn ** 0.5 / ref["grad_norm"] - 1):.2e} (bound {b_g:.1e})')
            assert ls == pytest.approx(ref['loss_source'], rel=b_s), use_plan
            assert lt == pytest.approx(ref['loss_target'], rel=b_t, abs=tol(FB, 'loss_target_abs')), use_plan
            assert gn ** 0.5 == pytest.approx(ref['grad_norm'], rel=b_g), use_plan
        if loss_t == 'ghm':         # the histograms of |p_y - 1| of the bf16 network: bins move by a few percent
            got = st.loss_fn_t.acc_sum.cpu().numpy()
            assert got.sum() == pytest.approx(float(ghm.acc_sum.sum()), rel=1e-2)
            np.testing.assert_allclose(got, ghm.acc_sum.numpy(), rtol=0.15, atol=0.05)
        if bct:                     # four EMA updates (two heads x two steps) on the pseudo labels
            torch.testing.assert_close(bt.freq.cpu(), bal.freq, rtol=0, atol=tol(FB, 'freq_t_abs', floor=2e-4))
    if loss_t in ('ohem', 'focal', 'ghm'):
        _captured_replay_matches_eager(model, protos, ones, g, loss_t)


def _captured_replay_matches_eager(model, protos, ones, g, loss_t):
    """No host-side balancer: the whole step can be captured.  Step 1 eager, then step 2 as a graph replay, against
    the same two steps eager: losses, gradient norm and GHM's state agree, and a further replay advances GHM's state."""
    from regda_amd.ssl import SSLStep
    args = (g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'])
    runs = []
    for captured in (False, True):
        m = model()
        m.set_drop_masks(ones.cuda(), ones.cuda())          # (device masks: nothing is copied from the host in capture)
        st = SSLStep(m, protos, loss_t=loss_t)
        st.step(*args, 1e-3)
        if captured:
            st.capture(*args)
        out = [float(x.item()) for x in st.step(*args, 1e-3)]
        acc = st.loss_fn_t.acc_sum.clone() if loss_t == 'ghm' else None
        runs.append((out, acc, st))
    (eager, acc_e, _), (graph, acc_g, st) = runs
    for a, b in zip(graph, eager):
        assert a == pytest.approx(b, rel=1e-5)
    if loss_t == 'ghm':
        torch.testing.assert_close(acc_g, acc_e, rtol=1e-5, atol=0)
        st.step(*args, 1e-3)
        assert not torch.equal(st.loss_fn_t.acc_sum, acc_g)


def test_source_and_align_steps_with_ohem_source_loss(monkeypatch):
    """SourceStep and AlignStep with loss_s='OhemCrossEntropy' against the CPU steps (source loss restated); the
    default SourceStep (loss_s='CrossEntropy') against the CPU step with the oracle's CE; AlignStep with
    loss_s='CrossEntropy' and a source balancer (--bcs) against the CPU step with the oracle's class-weighted CE."""
    from oracle import model as omodel
    from oracle.step import CpuAlignStep
    from regda_amd.align import AlignStep
    from regda_amd.gast.balance import ClassBalance
    from regda_amd.source import SourceStep
    rt, sd, b, protos, ones, model = _shallow()
    g = {k: v.cuda() for k, v in b.items()}
    for loss_s, kind in (('OhemCrossEntropy', 'ohem'), ('CrossEntropy', 'ce')):
        # stage 1: model(src) -> loss_calc -> backward (no alignment)
        w = {k: v.clone() for k, v in sd.items()}
        names = omodel.param_names(w)
        for k in names:
            w[k].requires_grad_(True)
        s1, s2, _ = omodel.forward(w, b['images_s'], True, (ones, ones), rt, {})
        ref = loss_ref.loss_calc([s1, s2], b['label_s'], loss_ref.make_loss(kind))
        grads = torch.autograd.grad(ref, [w[k] for k in names], allow_unused=True)
        gn_ref = torch.sqrt(sum((gg.double() ** 2).sum() for gg in grads if gg is not None)).item()
        st = SourceStep(model(), loss_s=loss_s)
        ls, _, gn = st.step(g['images_s'], g['label_s'], None, 1e-3)
        assert ls.item() == pytest.approx(float(ref), rel=STEP_LOSS_REL), loss_s
        assert gn.sqrt().item() == pytest.approx(gn_ref, rel=STEP_GN_REL), loss_s
        if kind == 'ohem':
            ref_ohem = float(ref)
        else:
            ref_ce = float(ref)
            assert abs(ref_ce - ref_ohem) > 0.05 * ref_ohem          # the two losses do differ here
    # stage 2
    f0s = torch.tensor([0.05, 0.05, 0.1, 0.1, 0.2, 0.5])
    for loss_s, balanced in (('OhemCrossEntropy', False), ('CrossEntropy', True)):
        bal = bal_ref = None
        if balanced:
            bal_ref, bal = olp.ClassBalanceState(6, -1, 0.5, 0.5), ClassBalance(6, -1, 0.5, 0.5)
            bal_ref.freq, bal.freq = f0s.clone(), f0s.cuda()
        else:
            _patch_oracle(monkeypatch, 'ohem', None)
        ref = CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, balancer_s=bal_ref).step(
            b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))
        monkeypatch.undo()
        st = AlignStep(model(), protos, loss_s=loss_s, class_balancer_s=bal)
        ls, la, gn = st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], 1e-3)
        assert ls.item() == pytest.approx(ref['loss_seg'], rel=STEP_LOSS_REL), loss_s
        assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=STEP_GN_REL), loss_s
        if balanced:
            assert abs(ref['loss_seg'] - ref_ce) > 0.05 * ref_ce         # the class weights do change the loss
            np.testing.assert_allclose(bal.freq.cpu().numpy(), bal_ref.freq.numpy(), rtol=1e-6)


@pytest.mark.parametrize('kind', ['focal', 'ce'])
def test_large_rows_raise_the_lds_limit(kind):
    """W = 2048: the gradient pass needs ~117 KB of dynamic LDS, above the 64 KB default (hipFuncSetAttribute); CE
    (CrossEntropy, rgda_upsample_ce) and focal (rgda_upsample_loss) run the same gradient pass."""
    from regda_amd.gast.balance import CrossEntropy
    g = torch.Generator().manual_seed(8)
    p1, p2 = torch.randn(1, 6, 32, 32, generator=g) * 2, torch.randn(1, 6, 32, 32, generator=g) * 2
    lab = torch.randint(-1, 6, (1, 128, 2048), generator=g)
    fn = loss_ref.make_loss(kind)
    r1, r2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    ref = loss_ref.loss_calc([r1, r2], lab, fn)
    ref.backward()
    ours = CrossEntropy(ignore_label=-1) if kind == 'ce' else fused(kind)
    loss, g1, g2 = run_fused(ours, kind, p1, p2, lab, None)
    assert float(loss) == pytest.approx(float(ref), rel=1e-5)
    np.testing.assert_allclose(g1.numpy(), r1.grad.numpy(), rtol=1e-3, atol=1e-4 * float(r1.grad.abs().max()))
