"""GPU: seven classes (the LoveDA tasks, configs/st/regda/2rural.py / 2urban.py) through every class-count-specific
kernel and the steps built on them.  Integer results bit for bit against the reference-minted goldens
(tests/golden/make_c7_goldens.py -> c7.npz) and the CPU oracle; float results within the tolerances the six-class tests
state for the same kernels; step-level bounds from tests/golden/c7_tolerances.json (derive_c7_tolerances.py)."""
import json
import os

import numpy as np
import pytest
import torch

import loss_ref
from oracle import labels as olab
from oracle import labelpath as opath
from oracle import model as omodel

pytestmark = pytest.mark.gpu

C = 7
HERE = os.path.dirname(os.path.abspath(__file__))
_TOL = json.load(open(os.path.join(HERE, 'golden', 'c7_tolerances.json')))


def tol(key, floor=1e-3):
    return max(_TOL['factor'] * _TOL['shallow_step_c7'][key], floor)


def tol_cos(key):
    return 1.0 - _TOL['factor'] * (1.0 - _TOL['shallow_step_c7'][key])


def tol_gn():
    return max(tol('grad_norm'), 0.5 * (1.0 - _TOL['shallow_step_c7']['grad_cos_global']))


def cu(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda()


def build(rt, ncls=C):
    from regda_amd.models.Encoder import Deeplabv2
    return Deeplabv2(dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True,
                          cascade=False, use_ppm=True, ppm=dict(num_classes=ncls, use_aux=False, fc_dim=2048),
                          inchannels=2048, num_classes=ncls, is_ins_norm=True))


def region_maps(rng, b, h, w, nreg):
    regs = np.zeros((b, h, w), np.int64)
    for i in range(b):
        for r in range(1, nreg + 1):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            regs[i, y0:y0 + rng.integers(1, max(2, h // 4)), x0:x0 + rng.integers(1, max(2, w // 4))] = r
    return regs


# ------------------------------------------------------------------------------------------------ label path, bit exact
def test_pseudo_select_c7_golden(gold):
    from regda_amd.gast.pseudo_generation import pseudo_selection
    g = gold('c7.npz')
    for i in range(int(g['ps_n'])):
        out = pseudo_selection(cu(g[f'ps_in{i}']), 0.8, 0.6, 'tensor', -1).cpu().numpy()
        assert np.array_equal(out, g[f'ps_out{i}'].astype(np.int64)), i
    # the full-size map (the SSL step's 8 x 512 x 512) against the oracle
    soft = torch.softmax(torch.randn(8, C, 512, 512, generator=torch.Generator().manual_seed(5)) * 3, 1)
    out = pseudo_selection(soft.cuda(), 0.8, 0.6, 'tensor', -1).cpu().numpy()
    assert np.array_equal(out, olab.pseudo_selection(soft.numpy(), 0.8, 0.6, -1))
    assert (out == 6).any()


def test_lrh_two_call_c7_golden(gold):
    from regda_amd.utils.local_region_homog import Homogenizer
    g = gold('c7.npz')
    for i in range(int(g['lrh_n'])):
        h = Homogenizer(percent=float(g[f'lrh_pct{i}']), class_num=C, ignore_label=-1)
        out = h(cu(g[f'lrh_lab{i}'], torch.int64), cu(g[f'lrh_reg{i}'], torch.int64)).cpu().numpy()
        assert np.array_equal(out, g[f'lrh_out{i}'].astype(np.int64)), i


def soft_for(lab):
    """Soft labels whose pseudo_selection is `lab` exactly: 0.9 on the labelled class (its threshold is 0.72), 0.1 / 6 on
    the others (below every threshold, >= 0.6), uniform 1 / 7 where lab = -1 (nothing passes)."""
    b, h, w = lab.shape
    soft = np.full((b, C, h, w), np.float32(0.1) / np.float32(6), np.float32)
    for c in range(C):
        soft[:, c][lab == c] = 0.9
    soft.transpose(0, 2, 3, 1)[lab == -1] = np.float32(1.0 / 7)
    return soft


def test_fused_pseudo_lrh_c7_golden(gold):
    """rgda_pseudo_lrh (the SSL step's fused select + LRH) at seven classes: the golden LRH cases fed as soft labels
    that select exactly the golden input labels (widths padded with region-0 ignore pixels to hw % 4 == 0), then a
    seeded full-size map against the two calls and the oracle."""
    from regda_amd import ops
    g = gold('c7.npz')
    for i in range(int(g['lrh_n'])):
        lab, regs = g[f'lrh_lab{i}'].astype(np.int64), g[f'lrh_reg{i}'].astype(np.int64)
        b, h, w = lab.shape
        pad = (-h * w) % 4 and next(p for p in range(1, 5) if (h * (w + p)) % 4 == 0)
        if pad:
            lab = np.concatenate([lab, np.full((b, h, pad), -1, np.int64)], 2)
            regs = np.concatenate([regs, np.zeros((b, h, pad), np.int64)], 2)
        sc = cu(soft_for(lab))
        out, _ = ops.pseudo_lrh(sc, sc.amax((2, 3)).contiguous(), cu(regs), 0.8, 0.6, float(g[f'lrh_pct{i}']), C, -1,
                                max_regions=4096)
        assert np.array_equal(out.cpu().numpy()[:, :, :w], g[f'lrh_out{i}'].astype(np.int64)), i
    rng = np.random.default_rng(7)
    b, h, w = 8, 512, 512
    gen = torch.Generator().manual_seed(11)
    blocks = torch.randn(b, C, 32, 32, generator=gen).repeat_interleave(16, 2).repeat_interleave(16, 3)
    soft = torch.softmax(3.0 * blocks + torch.randn(b, C, h, w, generator=gen), 1).contiguous()
    regs = region_maps(rng, b, h, w, 250)
    sc, rc = soft.cuda(), torch.from_numpy(regs).cuda()
    out, _ = ops.pseudo_lrh(sc, sc.amax((2, 3)).contiguous(), rc, 0.8, 0.6, 0.5, C, -1, max_regions=4096)
    two = ops.lrh(ops.pseudo_select(sc, 0.8, 0.6, -1), rc, 0.5, C, -1, max_regions=4096)
    assert torch.equal(out, two)
    want = olab.homogenize(olab.pseudo_selection(soft.numpy(), 0.8, 0.6, -1), regs, 0.5, C, -1)
    assert np.array_equal(out.cpu().numpy(), want) and (want == 6).any()


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events()}


def test_downscale_label_c7_fast_kernel_golden(gold):
    """rgda_proto_stats at b = 8, 512 x 512 (the step's shape) and seven classes: label_ds bit for bit against the
    reference's DownscaleLabel (ratio exactly 0.75, a class tied with ignore, an all-ignore cell, class 6 winning), the
    prototype sums / counts against the oracle, and the launch is the fast scale-16 kernel (before, seven classes could
    only be served by the one-workgroup-per-cell kernel)."""
    import sys
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from make_c7_goldens import checksum, downscale_big_input
    from regda_amd import ops
    g = gold('c7.npz')
    lab = downscale_big_input()
    assert checksum(lab) == g['ds_big_sum']
    feat = torch.randn(8, 64, 32, 32, generator=torch.Generator().manual_seed(3))
    res = {}

    def run():
        res['stats'], res['ds'] = ops.proto_stats(feat.cuda(), cu(lab), 16, -1, 0.75, C)
    names = _kernel_names(run)
    assert any('downscale_label16_kernel' in n for n in names), sorted(n for n in names if 'kernel' in n)
    assert not any(n.startswith('downscale_label_kernel') for n in names)
    ds = res['ds'].cpu()
    assert np.array_equal(ds.numpy().reshape(8, 32, 32), g['ds_big_out'].astype(np.int64).reshape(8, 32, 32))
    sums, cnt = opath.prototype_statistics(feat, ds, C, -1)
    st = res['stats'].cpu()
    assert torch.equal(st[C * 64:C * 64 + C], cnt.reshape(-1).float())
    np.testing.assert_allclose(st[:C * 64].reshape(C, 64).numpy(), sums.reshape(C, 64).numpy(), rtol=1e-5, atol=1e-5)
    assert int(st[C * 64 + C:C * 64 + C + 1].view(torch.int32)) == 0


# ------------------------------------------------------------------------------------------------ float kernels
def test_classifier_fwd_bwd_c7():
    from regda_amd import ops
    gen = torch.Generator().manual_seed(4)
    N, HW, K = 2, 32 * 32, 512
    hid = (torch.randn(N * HW, K, generator=gen)).to(torch.bfloat16).cuda()
    w, bias = torch.randn(C, K, generator=gen) * 0.05, torch.randn(C, generator=gen)
    logits = torch.empty(N, C, HW, device='cuda')
    ops.classifier_fwd(hid, w.cuda(), bias.cuda(), logits, N, HW, K, C)
    h32 = hid.float().cpu()
    ref = (h32 @ w.t() + bias).reshape(N, HW, C).permute(0, 2, 1)
    np.testing.assert_allclose(logits.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4)
    gl = torch.randn(N, C, HW, generator=gen)
    dh = torch.empty(N * HW, K, dtype=torch.bfloat16, device='cuda')
    dw, db = torch.zeros(C, K, device='cuda'), torch.zeros(C, device='cuda')
    ops.classifier_bwd(hid, w.cuda(), gl.cuda(), dh, dw, db, N, HW, K, C)
    g2 = gl.permute(0, 2, 1).reshape(N * HW, C)
    np.testing.assert_allclose(dh.float().cpu().numpy(), (g2 @ w).numpy(), rtol=1e-2, atol=1e-2)
    np.testing.assert_allclose(dw.cpu().numpy(), (g2.t() @ h32).numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(db.cpu().numpy(), g2.sum(0).numpy(), rtol=1e-4, atol=1e-4)


def test_teacher_probs_c7():
    from regda_amd import ops
    g = torch.Generator().manual_seed(8)
    p1, p2 = torch.randn(2, C, 32, 32, generator=g) * 3, torch.randn(2, C, 32, 32, generator=g) * 3
    ref = opath.teacher_probs(p1, p2, (512, 512))
    out = ops.teacher_probs(p1.cuda(), p2.cuda(), (512, 512)).cpu()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)


def test_label_refine_c7_with_and_without_superpixels():
    from regda_amd.gast.alignment import Aligner
    g = torch.Generator().manual_seed(11)
    b, k, h, w, H = 2, 2048, 32, 32, 512
    feat = torch.randn(b, k, h, w, generator=g)
    protos = torch.randn(C, k, generator=g)
    p1, p2 = torch.randn(b, C, h, w, generator=g) * 2, torch.randn(b, C, h, w, generator=g) * 2
    soft = torch.softmax(torch.randn(b, C, H, H, generator=g) * 3, 1)
    al = Aligner(None, feat_channels=k, class_num=C, ignore_label=-1, decay=0.996)
    al.prototypes = protos.cuda()
    ref = opath.label_refine(feat, protos, [p1, p2], soft)
    out = al.label_refine(None, feat.cuda(), [p1.cuda(), p2.cuda()], soft.cuda(), True, 'all', 2.0).cpu()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=5e-4, atol=1e-6)
    cm = al._classmax_ws[:b * C * 4].view(torch.float32).cpu().reshape(b, C)
    assert torch.equal(cm, out.flatten(2).max(-1)[0])
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(H), indexing='ij')
    jit = torch.randint(-3, 4, (b, H, H), generator=g)
    sup = (((yy + jit).clamp(0, H - 1) // 16) * 32 + (xx + jit.flip(-1)).clamp(0, H - 1) // 16).long()
    sup[1, 300:340, 100:200] = 1088
    sup = sup.reshape(b, 1, H, H)
    for mode in ('all', 's'):
        ref = opath.label_refine(feat, protos, [p1, p2], soft, True, mode, 2.0, label_t_sup=sup)
        out = al.label_refine(sup.cuda(), feat.cuda(), [p1.cuda(), p2.cuda()], soft.cuda(), True, mode, 2.0).cpu()
        np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=5e-4, atol=1e-6, err_msg=mode)


def loss_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    b, h, H = 2, 32, 256
    p1, p2 = torch.randn(b, C, h, h, generator=g) * 2, torch.randn(b, C, h, h, generator=g) * 2
    lab = torch.randint(-1, C, (b, H, H), generator=g)
    soft = torch.softmax(torch.randn(b, C, H, H, generator=g) * 3, 1)
    return p1, p2, lab, soft


def fused7(kind, bal=None):
    from regda_amd.gast import balance as B
    if kind == 'ce':
        return B.CrossEntropy(ignore_label=-1, class_balancer=bal)
    if kind == 'ohem':
        return B.OhemCrossEntropy(ignore_label=-1, class_balancer=bal)
    if kind == 'focal':
        return B.FocalLoss(gamma=2.0, reduction='mean', ignore_label=-1)
    if kind == 'ghm':
        return B.GHMLoss(bins=30, momentum=0.99, ignore_label=-1)
    if kind == 'ups':
        return B.UPSLoss(threshold=0.7, class_balancer=bal, class_num=C, ignore_label=-1)
    return B.UVEMLoss(m=0.2, threshold=0.7, gamma=4.0, class_balancer=bal, class_num=C, ignore_label=-1)


@pytest.mark.parametrize('kind,balanced', [('ce', False), ('ce', True), ('ohem', False), ('focal', False),
                                           ('ghm', False), ('ups', False), ('ups', True), ('uvem', False), ('uvem', True)])
def test_upsample_losses_c7(kind, balanced):
    """upsample_ce and every upsample_loss kind at seven classes: loss and both logit gradients against
    tests/loss_ref.py (pixels near a decision boundary of the loss ignored on both sides, as the six-class tests do)."""
    from regda_amd.gast.balance import ClassBalance, loss_calc_uvem
    from regda_amd.utils.tools import loss_calc
    from test_losses_gpu import ignore_near_boundary
    p1, p2, lab, soft = loss_inputs(5)
    if kind not in ('ce', 'focal'):
        lab, _, n = ignore_near_boundary(kind, p1, p2, lab, soft)
        assert n < 0.002 * lab.numel()
    freq = torch.tensor([0.3, 0.2, 0.15, 0.1, 0.1, 0.1, 0.05])
    bal = ref_bal = None
    if balanced:
        bal = ClassBalance(C, -1, 0.9, 2.0)
        bal.freq = freq.cuda()
        ref_bal = opath.ClassBalanceState(C, -1, 0.9, 2.0)
        ref_bal.freq = freq.clone()
    st = loss_ref.GhmState(0.99)
    r1, r2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    ref = loss_ref.loss_calc([r1, r2], lab, loss_ref.make_loss(kind, balancer=ref_bal, ghm_state=st), soft)
    ref.backward()
    fn = fused7(kind, bal)
    q1, q2 = p1.cuda().requires_grad_(True), p2.cuda().requires_grad_(True)
    if kind in ('ups', 'uvem'):
        loss = loss_calc_uvem([q1, q2], lab.cuda(), soft.cuda(), fn, multi=True)
    else:
        loss = loss_calc([q1, q2], lab.cuda(), fn, multi=True)
    loss.backward()
    assert float(loss) == pytest.approx(float(ref), rel=1e-5)
    for got, want in ((q1.grad.cpu(), r1.grad), (q2.grad.cpu(), r2.grad)):
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-3, atol=1e-4 * float(want.abs().max()))
    if kind == 'ghm':
        np.testing.assert_allclose(fn.acc_sum.cpu().numpy(), st.acc_sum.numpy(), rtol=1e-5)
    if balanced:
        np.testing.assert_allclose(bal.freq.cpu().numpy(), ref_bal.freq.numpy(), rtol=1e-5)


def test_pcl_loss_c7():
    from regda_amd import ops
    g = torch.Generator().manual_seed(2)
    b, K, h, w = 2, 2048, 32, 32
    feat = torch.randn(b, K, h, w, generator=g)
    lab = torch.randint(-1, C, (b, h, w), generator=g)
    protos = torch.randn(C, K, generator=g)
    f = feat.clone().requires_grad_(True)
    ref = opath.prototype_contrastive_loss(protos, f, lab, 8.0, -1)
    ref.backward()
    dfeat = torch.zeros(b * h * w, K, dtype=torch.bfloat16, device='cuda')
    loss = ops.pcl_loss(feat.cuda(), lab.cuda(), protos.cuda(), temperature=8.0, dfeat=dfeat)
    # the bounds of tests/test_align_gpu.py::test_pcl_loss_production_shape_weight_and_accumulate
    assert abs(float(loss) - ref.item()) <= 2e-5 * abs(ref.item())
    want = f.grad.permute(0, 2, 3, 1).reshape(b * h * w, K)
    assert ((dfeat.float().cpu() - want).norm() / want.norm()).item() < 3e-3


# ------------------------------------------------------------------------------------------------ steps
def test_ssl_step_c7_matches_the_oracle_step():
    """resnet17t SSLStep at seven classes (fused select + LRH included) against oracle.step.CpuStep(class_num=7), the
    fixture of derive_c7_tolerances.py; bounds: three rounding-noise units of it."""
    from oracle.step import CpuStep
    from regda_amd.ssl import SSLStep
    import sys
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from derive_c7_tolerances import shallow_c7_inputs
    rt, sd, b, protos, ones = shallow_c7_inputs()
    cpu = CpuStep(sd, protos, resnet_type=rt, class_num=C, lr=1e-3)
    ref = cpu.step(b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'], (ones, ones), (ones, ones))
    m = build(rt)
    m.load_state_dict(sd, strict=True)
    m.set_drop_masks(ones, ones)
    st = SSLStep(m, protos, class_num=C)
    g = {k: v.cuda() for k, v in b.items()}
    ls, lt, gn = st.step(g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'], 1e-3)
    hard = st.last_hard.cpu().numpy()
    assert ls.item() == pytest.approx(ref['loss_source'], rel=tol('loss_source'))
    assert lt.item() == pytest.approx(ref['loss_target'], rel=tol('loss_target'), abs=tol('loss_target_abs'))
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=tol_gn())
    assert (hard != ref['hard'].numpy()).mean() < tol('hard_mismatch') and (hard == 6).any()
    assert st.lrh_flag() == 0
    assert ((st.prototypes.cpu() - cpu.prototypes).norm() / cpu.prototypes.norm()).item() < tol('protos_rel', floor=1e-4)
    k = 'encoder.resnet.conv1.weight'
    d_ref, d_got = cpu.sd[k].detach() - sd[k], dict(m.named_parameters())[k].detach().cpu() - sd[k]
    cos = (d_ref.flatten() @ d_got.flatten() / (d_ref.norm() * d_got.norm())).item()
    assert cos > tol_cos('stem_update_cos')
    assert d_got.norm().item() == pytest.approx(d_ref.norm().item(), rel=tol('stem_update_norm_dev', floor=5e-3))


def test_align_step_c7_matches_the_oracle_stage2_step():
    """AlignStep at seven classes against oracle.step.CpuAlignStep(class_num=7), with the bounds of the six-class test
    (tests/test_align_gpu.py)."""
    from oracle.step import CpuAlignStep
    from regda_amd.align import AlignStep
    from regda_amd.synthetic import make_batch
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, C, seed=6)
    b = make_batch(b=4, size=128, classes=C, seed=11, device='cpu')
    protos = torch.randn(C, 2048, generator=torch.Generator().manual_seed(1))
    ones = torch.ones(4, 512)
    cpu = CpuAlignStep(sd, protos, resnet_type=rt, class_num=C, lr=1e-3, proto_decay=0.999)
    ref = cpu.step(b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))
    m = build(rt)
    m.load_state_dict(sd, strict=True)
    m.set_drop_masks(ones, ones)
    st = AlignStep(m, protos, class_num=C)
    g = {k: v.cuda() for k, v in b.items()}
    lseg, lal, gn = st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], 1e-3)
    assert lseg.item() == pytest.approx(ref['loss_seg'], rel=0.02)
    assert lal.item() == pytest.approx(ref['loss_align'], rel=0.02)
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)
    assert torch.equal(st.last_label_s_down.cpu(), ref['label_s_down'])
    assert ((st.prototypes.cpu() - cpu.prototypes).norm() / cpu.prototypes.norm()).item() < 2e-3
    # the target labels come from the student's own bf16 predictions: near-uniform seven-class probabilities at the
    # selection thresholds, then whole LRH regions that follow their majority, move more pixels than at six classes
    # (every kernel of that chain is bit exact or within its fp32 bound at seven classes above); stated bounds
    hm = (st.last_hard.cpu() != ref['hard']).float().mean().item()
    lm = (st.last_label_t.cpu() != ref['label_t']).float().mean().item()
    print('[align step c7] hard mismatch %.4f label_t mismatch %.4f' % (hm, lm))
    assert hm < 0.1 and lm < 0.12


def test_source_step_c7_matches_the_composed_oracle():
    """SourceStep(align_domain=True) at seven classes against the CPU stage-1 step composed from oracle pieces
    (tests/test_coral_gpu.py::cpu_stage1), with that test's bounds."""
    from regda_amd.source import SourceStep
    from regda_amd.synthetic import make_batch
    from test_coral_gpu import cpu_stage1
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, C, seed=6)
    bb = make_batch(b=2, size=128, classes=C, seed=11, device='cpu')
    xs, lab, xt = bb['images_s'], bb['label_s'], bb['images_t']
    ones = torch.ones(2, 512)
    ref = cpu_stage1(sd, rt, xs, lab, xt, (ones, ones), (ones, ones))
    m = build(rt)
    m.load_state_dict(sd, strict=True)
    m.set_drop_masks(ones, ones)
    st = SourceStep(m, align_domain=True, class_num=C)
    ls, ld, gn = st.step(xs.cuda(), lab.cuda(), xt.cuda(), lr=1e-3)
    assert ld.item() == pytest.approx(ref['loss_domain'], rel=0.05)
    assert ls.item() == pytest.approx(ref['loss_seg'], rel=0.02)
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)


def test_c7_step_is_bit_reproducible_and_plan_replay_matches_eager():
    """Two identical seven-class runs give bit-identical weights, losses and masks; record_plan() replay equals the
    eager step."""
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, C, seed=12)
    ones = torch.ones(4, 512)
    b1 = make_batch(b=2, size=128, classes=C, seed=21)
    b2 = make_batch(b=2, size=128, classes=C, seed=22)
    seq, lrs = [b1, b1, b2, b1], [1e-3, 1e-3, 2e-3, 1e-3]

    def run(use_plan):
        m = build(rt)
        m.load_state_dict(sd, strict=True)
        m.set_drop_masks(ones, ones)
        st = SSLStep(m, torch.randn(C, 2048, generator=torch.Generator().manual_seed(5)), class_num=C, ema_decay=0.9)
        out, hards = [], []
        for i, (b, lr) in enumerate(zip(seq, lrs)):
            if use_plan and i == 1:
                st.record_plan(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'])
                out.append([float(x.item()) for x in st._out])
            else:
                o = st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], lr)
                out.append([float(x.item()) for x in o])
            hards.append(st.last_hard.clone())
        torch.cuda.synchronize()
        return m, st, out, hards

    runs = [run(False), run(False), run(True)]
    (m0, s0, o0, h0), (m1, s1, o1, h1), (mp, sp, op, hp) = runs
    assert o0 == o1 and torch.equal(m0.flat_p, m1.flat_p) and torch.equal(m0.flat_buf, m1.flat_buf)
    assert all(torch.equal(a, b) for a, b in zip(h0, h1))
    assert torch.equal(s0.prototypes, s1.prototypes)
    assert sp._plan is not None
    assert op == o0 and torch.equal(mp.flat_p, m0.flat_p) and torch.equal(sp.teacher.flat_p, s0.teacher.flat_p)
    assert all(torch.equal(a, b) for a, b in zip(hp, h0))


def test_resnet50_online_teacher_step_and_eval_on_a_loveda_tile(tmp_path):
    """The LoveDA recipe's shapes: resnet50 (MODEL = 'ResNet'), 8 + 8 images of 512 x 512, seven classes, the online EMA
    teacher; then gener_target_pseudo (8-view TTA, sliding window) and evaluate on one 1024 x 1024 tile."""
    from regda_amd.gast.pseudo_generation import gener_target_pseudo
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    from regda_amd.utils.eval import evaluate
    from regda_amd.utils.tools import import_config
    cfg = import_config('st.regda.2rural', create=False, copy=False)
    rt = 'resnet50'
    m = build(rt, cfg.NUM_CLASSES)
    m.load_state_dict(omodel.init_state_dict(rt, C, seed=3), strict=True)
    b = make_batch(b=8, size=512, classes=C, seed=4, with_soft=False)
    st = SSLStep(m, torch.randn(C, 2048, generator=torch.Generator().manual_seed(2)), class_num=cfg.NUM_CLASSES,
                 ignore_label=cfg.IGNORE_LABEL, ema_decay=0.999)
    for _ in range(2):
        ls, lt, gn = st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)
    assert all(np.isfinite(x.item()) for x in (ls, lt, gn)) and st.lrh_flag() == 0
    hard = st.last_hard
    assert hard.shape == (8, 512, 512) and int(hard.min()) >= -1 and int(hard.max()) <= 6
    tile = torch.randn(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(9))
    gener_target_pseudo(cfg, m, [(tile, {'fname': ['t0.png']})], str(tmp_path), slide=True, save_prob=True,
                        size=(1024, 1024), ignore_label=-1)
    probs = torch.load(os.path.join(str(tmp_path), 't0.png.pt'))
    assert tuple(probs.shape) == (C, 1024, 1024) and torch.isfinite(probs).all()
    np.testing.assert_allclose(probs.sum(0).numpy(), 1.0, rtol=0, atol=1e-4)
    gt = torch.randint(-1, C, (1, 1024, 1024), generator=torch.Generator().manual_seed(1))
    res = evaluate(m, cfg, is_training=True, dataloader=[(tile, {'cls': gt})], slide=True, tta=False)
    assert res is not None
