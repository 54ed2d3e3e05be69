"""GPU: 8, 11 and 16 classes (OpenEarthMap / UAVid, an odd count, iSAID / GID-15 with background) through every
class-count-specific kernel and the steps built on them.  Integer results bit for bit against the reference-minted goldens
(tests/golden/make_cn_goldens.py -> cn.npz) and the CPU oracle; float results within the tolerances the six- and
seven-class tests state for the same kernels; the SSL step within tests/golden/cn_tolerances.json
(derive_cn_tolerances.py, at 16 classes), the stage-1 / stage-2 steps with the bounds of the seven-class tests.  Before 6 <= C <= 16 every one of these counts returned RGDA_ERR_UNSUPPORTED."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import loss_ref
from oracle import labels as olab
from oracle import labelpath as opath
from oracle import model as omodel

pytestmark = pytest.mark.gpu

COUNTS = (8, 11, 16)
HERE = os.path.dirname(os.path.abspath(__file__))
_TOL = json.load(open(os.path.join(HERE, 'golden', 'cn_tolerances.json')))


def tol(key, floor=1e-3):
    return max(_TOL['factor'] * _TOL['shallow_step_c16'][key], floor)


def tol_cos(key):
    return 1.0 - _TOL['factor'] * (1.0 - _TOL['shallow_step_c16'][key])


def tol_gn():
    return max(tol('grad_norm'), 0.5 * (1.0 - _TOL['shallow_step_c16']['grad_cos_global']))


@pytest.fixture(scope='module')
def cn():
    return np.load(os.path.join(HERE, 'golden', 'cn.npz'))


def cu(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda()


def build(rt, ncls):
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
@pytest.mark.parametrize('C', COUNTS)
def test_pseudo_select_golden(cn, C):
    from regda_amd.gast.pseudo_generation import pseudo_selection
    p = f'c{C}_'
    for i in range(int(cn[p + 'ps_n'])):
        out = pseudo_selection(cu(cn[f'{p}ps_in{i}']), 0.8, 0.6, 'tensor', -1).cpu().numpy()
        assert np.array_equal(out, cn[f'{p}ps_out{i}'].astype(np.int64)), i
    soft = torch.softmax(torch.randn(8, C, 512, 512, generator=torch.Generator().manual_seed(5)) * 3, 1)
    out = pseudo_selection(soft.cuda(), 0.8, 0.6, 'tensor', -1).cpu().numpy()
    assert np.array_equal(out, olab.pseudo_selection(soft.numpy(), 0.8, 0.6, -1))
    assert (out == C - 1).any()


@pytest.mark.parametrize('C', COUNTS)
def test_lrh_two_call_golden(cn, C):
    from regda_amd.utils.local_region_homog import Homogenizer
    p = f'c{C}_'
    for i in range(int(cn[p + 'lrh_n'])):
        h = Homogenizer(percent=float(cn[f'{p}lrh_pct{i}']), class_num=C, ignore_label=-1)
        out = h(cu(cn[f'{p}lrh_lab{i}'], torch.int64), cu(cn[f'{p}lrh_reg{i}'], torch.int64)).cpu().numpy()
        assert np.array_equal(out, cn[f'{p}lrh_out{i}'].astype(np.int64)), i


def soft_for(lab, C):
    """Soft labels whose pseudo_selection is `lab` exactly: 0.9 on the labelled class (its threshold is 0.72), 0.1 / (C-1)
    on the others (below every threshold), uniform 1 / C where lab = -1 (nothing passes)."""
    b, h, w = lab.shape
    soft = np.full((b, C, h, w), np.float32(0.1) / np.float32(C - 1), np.float32)
    for c in range(C):
        soft[:, c][lab == c] = 0.9
    soft.transpose(0, 2, 3, 1)[lab == -1] = np.float32(1.0 / C)
    return soft


@pytest.mark.parametrize('C', COUNTS)
def test_fused_pseudo_lrh_golden(cn, C):
    """rgda_pseudo_lrh (the SSL step's fused select + LRH): the golden LRH cases fed as soft labels that select exactly
    the golden input labels, then a seeded full-size map against the two calls and the oracle."""
    from regda_amd import ops
    p = f'c{C}_'
    for i in range(int(cn[p + 'lrh_n'])):
        lab, regs = cn[f'{p}lrh_lab{i}'].astype(np.int64), cn[f'{p}lrh_reg{i}'].astype(np.int64)
        b, h, w = lab.shape
        pad = (-h * w) % 4 and next(q for q in range(1, 5) if (h * (w + q)) % 4 == 0)
        if pad:
            lab = np.concatenate([lab, np.full((b, h, pad), -1, np.int64)], 2)
            regs = np.concatenate([regs, np.zeros((b, h, pad), np.int64)], 2)
        sc = cu(soft_for(lab, C))
        out, _ = ops.pseudo_lrh(sc, sc.amax((2, 3)).contiguous(), cu(regs), 0.8, 0.6, float(cn[f'{p}lrh_pct{i}']), C, -1,
                                max_regions=4096)
        assert np.array_equal(out.cpu().numpy()[:, :, :w], cn[f'{p}lrh_out{i}'].astype(np.int64)), i
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
    assert np.array_equal(out.cpu().numpy(), want) and (want == C - 1).any()


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events()}


@pytest.mark.parametrize('C', COUNTS)
def test_downscale_label_fast_kernel_golden(cn, C):
    """rgda_proto_stats at b = 8, 512 x 512 (the step's shape): label_ds bit for bit against the reference's
    DownscaleLabel, the prototype sums / counts against the oracle, the launch is the single-pass scale-16 kernel (not
    the one-workgroup-per-cell one), and below min_ratio 0.5 the tie rule matches the oracle's."""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from make_cn_goldens import checksum, downscale_big_input
    from regda_amd import ops
    lab = downscale_big_input(C)
    assert checksum(lab) == cn[f'c{C}_ds_big_sum']
    feat = torch.randn(8, 64, 32, 32, generator=torch.Generator().manual_seed(3))
    res = {}

    def run():
        res['stats'], res['ds'] = ops.proto_stats(feat.cuda(), cu(lab), 16, -1, 0.75, C)
    names = _kernel_names(run)
    assert any('downscale_label16' in n for n in names), sorted(n for n in names if 'kernel' in n)
    assert not any('downscale_label_kernel' in n for n in names)
    ds = res['ds'].cpu()
    assert np.array_equal(ds.numpy().reshape(8, 32, 32), cn[f'c{C}_ds_big_out'].astype(np.int64).reshape(8, 32, 32))
    sums, cnt = opath.prototype_statistics(feat, ds, C, -1)
    st = res['stats'].cpu()
    assert torch.equal(st[C * 64:C * 64 + C], cnt.reshape(-1).float())
    np.testing.assert_allclose(st[:C * 64].reshape(C, 64).numpy(), sums.reshape(C, 64).numpy(), rtol=1e-5, atol=1e-5)
    assert int(st[C * 64 + C:C * 64 + C + 1].view(torch.int32)) == 0
    _, ds5 = ops.proto_stats(feat.cuda(), cu(lab), 16, -1, 0.5, C)
    want5 = np.asarray(olab.downscale_label(lab, 16, C, -1, 0.5)).reshape(8, 32, 32)
    assert np.array_equal(ds5.cpu().numpy().reshape(8, 32, 32), want5)
    assert want5[0, 0, 2] == 3 and want5[0, 0, 8] == C - 1          # classes tied with ignore win


# ------------------------------------------------------------------------------------------------ float kernels
@pytest.mark.parametrize('C', COUNTS)
def test_classifier_fwd_bwd(C):
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


@pytest.mark.parametrize('C', COUNTS)
def test_teacher_probs(C):
    from regda_amd import ops
    g = torch.Generator().manual_seed(8)
    p1, p2 = torch.randn(2, C, 32, 32, generator=g) * 3, torch.randn(2, C, 32, 32, generator=g) * 3
    ref = opath.teacher_probs(p1, p2, (512, 512))
    out = ops.teacher_probs(p1.cuda(), p2.cuda(), (512, 512)).cpu()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('C', COUNTS)
def test_label_refine_with_and_without_superpixels(C):
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


def fused(kind, C, bal=None):
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


@pytest.mark.parametrize('C', COUNTS)
@pytest.mark.parametrize('kind,balanced', [('ce', False), ('ce', True), ('ohem', False), ('ohem', True), ('focal', False),
                                           ('ghm', False), ('ups', False), ('ups', True), ('uvem', False), ('uvem', True)])
def test_upsample_losses(C, kind, balanced):
    """upsample_ce and every upsample_loss kind: loss and both logit gradients against tests/loss_ref.py (pixels near a
    decision boundary of the loss ignored on both sides, as the six-class tests do)."""
    from regda_amd.gast.balance import ClassBalance, loss_calc_uvem
    from regda_amd.utils.tools import loss_calc
    from test_losses_gpu import ignore_near_boundary
    g = torch.Generator().manual_seed(5)
    b, h, H = 2, 32, 256
    p1, p2 = torch.randn(b, C, h, h, generator=g) * 2, torch.randn(b, C, h, h, generator=g) * 2
    lab = torch.randint(-1, C, (b, H, H), generator=g)
    soft = torch.softmax(torch.randn(b, C, H, H, generator=g) * 3, 1)
    if kind not in ('ce', 'focal'):
        lab, _, n = ignore_near_boundary(kind, p1, p2, lab, soft)
        assert n < 0.002 * lab.numel()
    freq = torch.linspace(2.0, 1.0, C)
    freq = freq / freq.sum()
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
    fn = fused(kind, C, bal)
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


@pytest.mark.parametrize('C', COUNTS)
def test_pcl_loss(C):
    """PrototypeContrastiveLoss at K = 2048 (from 15 classes on, the kernel's 8-slice layout), with the bounds of
    tests/test_align_gpu.py::test_pcl_loss_production_shape_weight_and_accumulate."""
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
    assert abs(float(loss) - ref.item()) <= 2e-5 * abs(ref.item())
    want = f.grad.permute(0, 2, 3, 1).reshape(b * h * w, K)
    assert ((dfeat.float().cpu() - want).norm() / want.norm()).item() < 3e-3


# ------------------------------------------------------------------------------------------------ steps
@pytest.mark.parametrize('C', COUNTS)
def test_align_step_matches_the_oracle_stage2_step(C):
    """AlignStep against oracle.step.CpuAlignStep(class_num=C), with the bounds of the seven-class test; the target
    labels (the student's own near-uniform bf16 predictions through selection and LRH) with looser stated bounds."""
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
    m = build(rt, C)
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
    hm = (st.last_hard.cpu() != ref['hard']).float().mean().item()
    lm = (st.last_label_t.cpu() != ref['label_t']).float().mean().item()
    print('[align step c%d] hard mismatch %.4f label_t mismatch %.4f' % (C, hm, lm))
    assert hm < 0.2 and lm < 0.25


@pytest.mark.parametrize('C', COUNTS)
def test_source_step_matches_the_composed_oracle(C):
    from regda_amd.source import SourceStep
    from regda_amd.synthetic import make_batch
    from test_coral_gpu import cpu_stage1
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, C, seed=6)
    bb = make_batch(b=2, size=128, classes=C, seed=11, device='cpu')
    xs, lab, xt = bb['images_s'], bb['label_s'], bb['images_t']
    ones = torch.ones(2, 512)
    ref = cpu_stage1(sd, rt, xs, lab, xt, (ones, ones), (ones, ones))
    m = build(rt, C)
    m.load_state_dict(sd, strict=True)
    m.set_drop_masks(ones, ones)
    st = SourceStep(m, align_domain=True, class_num=C)
    ls, ld, gn = st.step(xs.cuda(), lab.cuda(), xt.cuda(), lr=1e-3)
    assert ld.item() == pytest.approx(ref['loss_domain'], rel=0.05)
    assert ls.item() == pytest.approx(ref['loss_seg'], rel=0.02)
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)


def test_c16_ssl_step_is_bit_reproducible_and_plan_replay_matches_eager():
    """resnet17t SSLStep at 16 classes (fused select + LRH): two identical runs give bit-identical weights, losses and
    masks; record_plan() replay equals the eager step."""
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    C, rt = 16, 'resnet17t'
    sd = omodel.init_state_dict(rt, C, seed=12)
    ones = torch.ones(4, 512)
    b1 = make_batch(b=2, size=128, classes=C, seed=21)
    b2 = make_batch(b=2, size=128, classes=C, seed=22)
    seq, lrs = [b1, b1, b2, b1], [1e-3, 1e-3, 2e-3, 1e-3]

    def run(use_plan):
        m = build(rt, C)
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

    (m0, s0, o0, h0), (m1, s1, o1, h1), (mp, sp, op, hp) = run(False), run(False), run(True)
    assert all(np.isfinite(v) for o in o0 for v in o)
    assert o0 == o1 and torch.equal(m0.flat_p, m1.flat_p) and torch.equal(m0.flat_buf, m1.flat_buf)
    assert all(torch.equal(a, b) for a, b in zip(h0, h1))
    assert torch.equal(s0.prototypes, s1.prototypes)
    assert sp._plan is not None
    assert op == o0 and torch.equal(mp.flat_p, m0.flat_p) and torch.equal(sp.teacher.flat_p, s0.teacher.flat_p)
    assert all(torch.equal(a, b) for a, b in zip(hp, h0))


def test_c16_resnet101_step_at_512():
    """resnet101, 8 + 8 images of 512 x 512, 16 classes: finite losses, labels in range, deterministic across two runs."""
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    C, rt = 16, 'resnet101'
    sd = omodel.init_state_dict(rt, C, seed=3)
    b = make_batch(b=8, size=512, classes=C, seed=4, with_soft=False)
    ones = torch.ones(16, 512)

    def run():
        m = build(rt, C)
        m.load_state_dict(sd, strict=True)
        m.set_drop_masks(ones, ones)                    # the heads' Dropout2d keep-masks, the same in both runs
        st = SSLStep(m, torch.randn(C, 2048, generator=torch.Generator().manual_seed(2)), class_num=C, ema_decay=0.999)
        out = [float(x.item()) for x in st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)]
        torch.cuda.synchronize()
        return out, st.last_hard.clone(), m.flat_p.clone(), st.lrh_flag()

    o0, h0, p0, f0 = run()
    o1, h1, p1, _ = run()
    assert all(np.isfinite(v) for v in o0) and f0 == 0
    assert h0.shape == (8, 512, 512) and int(h0.min()) >= -1 and int(h0.max()) <= C - 1
    assert o0 == o1 and torch.equal(h0, h1) and torch.equal(p0, p1)


def test_c16_1024_tiles_are_refused_before_the_step():
    """The fused upsample + loss row pass does not fit 16 classes at 1024-pixel rows: the step refuses at its first
    call, before any launch, and names the limit; 15 classes are served there (checked on the shapes only)."""
    from regda_amd import ops
    from regda_amd.ssl import SSLStep
    C, rt = 16, 'resnet17t'
    m = build(rt, C)
    m.load_state_dict(omodel.init_state_dict(rt, C, seed=1), strict=True)
    st = SSLStep(m, torch.randn(C, 2048), class_num=C)
    x = torch.zeros(1, 3, 1024, 1024, device='cuda')
    before = m.flat_p.clone()
    with pytest.raises(ValueError, match='W <= 1008'):
        st.step(x, torch.zeros(1, 1024, 1024, dtype=torch.int64, device='cuda'), x, None, None, 1e-3)
    assert torch.equal(m.flat_p, before)
    ops.check_step_shape(15, 2048, 1024, 1024)
    with pytest.raises(ValueError, match='6 <= class_num <= 16'):
        SSLStep(build(rt, 6), torch.randn(17, 2048), class_num=17)


@pytest.mark.parametrize('C', COUNTS)
def test_evaluate_confusion_matrix(C):
    """The confusion matrix `evaluate` accumulates (rgda_confusion_accumulate) at C classes, against numpy.  (The ASPP
    heads at C classes, 72 * C columns, run in every step test above.)"""
    from regda_amd import ops
    g = torch.Generator().manual_seed(3)
    yt = torch.randint(-1, C, (2, 64, 64), generator=g)
    yp = torch.randint(0, C, (2, 64, 64), generator=g)
    cm = torch.zeros(C, C, dtype=torch.int64, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.confusion_accumulate(yt.cuda(), yp.cuda(), cm, flag)
    keep = yt.numpy() >= 0
    want = np.zeros((C, C), np.int64)
    np.add.at(want, (yt.numpy()[keep], yp.numpy()[keep]), 1)
    assert np.array_equal(cm.cpu().numpy(), want) and int(flag.item()) == 0


# ------------------------------------------------------------------------------------------------ reference goldens
@pytest.mark.parametrize('C', COUNTS)
def test_label_refine_reference_golden(cn, C):
    """label_refine (mode 'all', without and with superpixels) against the reference's Aligner at C classes, within the
    bound of the six-class golden test."""
    from regda_amd.gast.alignment import Aligner
    p = f'c{C}_'
    g = {k[len(p):]: cn[k] for k in cn.files if k.startswith(p + 'rf_')}
    k = g['rf_feat'].shape[1]
    al = Aligner(None, feat_channels=k, class_num=C, ignore_label=-1, decay=0.996)
    al.prototypes = cu(g['rf_protos'])
    feat, p1, p2, soft = cu(g['rf_feat']), cu(g['rf_p1']), cu(g['rf_p2']), cu(g['rf_soft'])
    out = al.label_refine(None, feat, [p1, p2], soft.clone(), True, 'all', 2.0).cpu().numpy()
    np.testing.assert_allclose(out, g['rf_out'], rtol=5e-4, atol=1e-6)
    H = g['rf_sup'].shape[-1]
    sup = cu(g['rf_sup'], torch.int64).reshape(-1, 1, H, H)
    out = al.label_refine(sup, feat, [p1, p2], soft.clone(), True, 'all', 2.0).cpu().numpy()
    np.testing.assert_allclose(out, g['rf_out_sup'], rtol=5e-4, atol=1e-6)


@pytest.mark.parametrize('C', COUNTS)
def test_pcl_loss_reference_golden(cn, C):
    from regda_amd import ops
    p = f'c{C}_'
    feat, lab = cn[p + 'pcl_feat'], cn[p + 'pcl_lab'].astype(np.int64)
    b, K, h, w = feat.shape
    dfeat = torch.zeros(b * h * w, K, dtype=torch.bfloat16, device='cuda')
    loss = ops.pcl_loss(cu(feat), cu(lab), cu(cn[p + 'pcl_protos']), temperature=8.0, dfeat=dfeat)
    ref = float(cn[p + 'pcl_loss'])
    assert abs(float(loss) - ref) <= 2e-5 * abs(ref)
    want = torch.from_numpy(cn[p + 'pcl_gfeat']).permute(0, 2, 3, 1).reshape(b * h * w, K)
    assert ((dfeat.float().cpu() - want).norm() / want.norm()).item() < 3e-3


# ------------------------------------------------------------------------------------------------ SSL step vs oracle
@pytest.mark.parametrize('C', COUNTS)
def test_ssl_step_matches_the_oracle_step(C):
    """resnet17t SSLStep (fused select + LRH) against oracle.step.CpuStep(class_num=C) on the fixture of
    derive_cn_tolerances.py; bounds: three rounding-noise units of it at 16 classes."""
    from oracle.step import CpuStep
    from regda_amd.ssl import SSLStep
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from derive_cn_tolerances import shallow_cn_inputs
    rt, sd, b, protos, ones = shallow_cn_inputs(C)
    cpu = CpuStep(sd, protos, resnet_type=rt, class_num=C, lr=1e-3)
    ref = cpu.step(b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'], (ones, ones), (ones, ones))
    m = build(rt, C)
    m.load_state_dict(sd, strict=True)
    m.set_drop_masks(ones, ones)
    st = SSLStep(m, protos, class_num=C)
    g = {k: v.cuda() for k, v in b.items()}
    ls, lt, gn = st.step(g['images_s'], g['label_s'], g['images_t'], g['soft_t'], g['regs_t'], 1e-3)
    hard = st.last_hard.cpu().numpy()
    print('[ssl step c%d] loss_s %.6g (%.6g) loss_t %.6g (%.6g) |g| %.6g (%.6g) hard mismatch %.5f' % (
        C, ls.item(), ref['loss_source'], lt.item(), ref['loss_target'], gn.sqrt().item(), ref['grad_norm'],
        (hard != ref['hard'].numpy()).mean()))
    assert ls.item() == pytest.approx(ref['loss_source'], rel=tol('loss_source'))
    assert lt.item() == pytest.approx(ref['loss_target'], rel=tol('loss_target'), abs=tol('loss_target_abs'))
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=tol_gn())
    assert (hard != ref['hard'].numpy()).mean() < tol('hard_mismatch') and (hard >= 0).any()
    assert st.lrh_flag() == 0
    assert ((st.prototypes.cpu() - cpu.prototypes).norm() / cpu.prototypes.norm()).item() < tol('protos_rel', floor=1e-4)
    k = 'encoder.resnet.conv1.weight'
    d_ref, d_got = cpu.sd[k].detach() - sd[k], dict(m.named_parameters())[k].detach().cpu() - sd[k]
    cos = (d_ref.flatten() @ d_got.flatten() / (d_ref.norm() * d_got.norm())).item()
    assert cos > tol_cos('stem_update_cos')
    assert d_got.norm().item() == pytest.approx(d_ref.norm().item(), rel=tol('stem_update_norm_dev', floor=5e-3))


# ------------------------------------------------------------------------------------------------ teacher, eval, heads, aug
def test_c16_online_teacher_step_teacher_pass_and_evaluate(tmp_path):
    """16 classes through the public entry points: resnet17t SSLStep with the online EMA teacher, gener_target_pseudo
    (8-view TTA, sliding window) and evaluate, whose confusion matrix and mIoU are recomputed here from its own
    predictions."""
    import types
    from regda_amd.gast.pseudo_generation import gener_target_pseudo
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    from regda_amd.utils.eval import evaluate
    C, rt = 16, 'resnet17t'
    m = build(rt, C)
    m.load_state_dict(omodel.init_state_dict(rt, C, seed=3), strict=True)
    b = make_batch(b=2, size=128, classes=C, seed=4, with_soft=False)
    st = SSLStep(m, torch.randn(C, 2048, generator=torch.Generator().manual_seed(2)), class_num=C, ema_decay=0.999)
    for _ in range(2):
        ls, lt, gn = st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)
    assert all(np.isfinite(x.item()) for x in (ls, lt, gn)) and st.lrh_flag() == 0
    assert int(st.last_hard.max()) <= C - 1
    cfg = types.SimpleNamespace(NUM_CLASSES=C, IGNORE_LABEL=-1, LABEL_OFFSET=-1, DATASETS='OtherDA')
    tile = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(9))   # one whole 512 window
    gener_target_pseudo(cfg, m, [(tile, {'fname': ['t0.png']})], str(tmp_path), slide=True, save_prob=True,
                        size=(512, 512), ignore_label=-1)
    probs = torch.load(os.path.join(str(tmp_path), 't0.png.pt'))
    assert tuple(probs.shape) == (C, 512, 512) and torch.isfinite(probs).all()
    np.testing.assert_allclose(probs.sum(0).numpy(), 1.0, rtol=0, atol=1e-4)
    gt = torch.randint(-1, C, (1, 512, 512), generator=torch.Generator().manual_seed(1))
    import regda_amd.utils.eval as ev
    seen = {}
    real = ev.PixelMetricIgnore

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen['metric'] = self
    ev.PixelMetricIgnore = Spy
    try:
        res = evaluate(m, cfg, is_training=True, dataloader=[(tile, {'cls': gt})], slide=True, tta=False)
    finally:
        ev.PixelMetricIgnore = real
    from regda_amd.utils.tools import pre_slide
    with torch.no_grad():
        pred = pre_slide(m, tile.cuda(), num_classes=C, tta=False).argmax(1).cpu()
    keep = gt >= 0
    want = np.zeros((C, C), np.int64)
    np.add.at(want, (gt[keep].numpy(), pred[keep].numpy()), 1)
    cm = seen['metric'].confusion_matrix()
    assert cm.shape == (C, C) and np.array_equal(np.asarray(cm), want)
    d = np.diag(want).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = d / (want.sum(0) + want.sum(1) - d)
    assert res is not None and np.isfinite(np.nanmean(iou))
    print('[eval c16] mIoU %s' % (res[1] if isinstance(res, tuple) else res,))


def test_c16_aspp_head_against_the_oracle():
    """The stacked ASPP head at 16 classes (72 * C = 1152 columns) composed from the C-ABI calls like the model does:
    forward, input gradient, filter and bias gradients against oracle.model.aspp_head (the bounds of
    tests/test_aspp_gpu.py)."""
    from regda_amd import ops
    BF, DIL, dev = torch.bfloat16, (6, 12, 18, 24), 'cuda'
    N, K, h, w, C = 2, 64, 20, 28, 16
    g = torch.Generator().manual_seed(16)
    rb = lambda t: t.to(BF).float()
    l2 = lambda a, b: ((a.float().cpu() - b.float().cpu()).norm() / (b.float().cpu().norm() + 1e-12)).item()
    x = rb(torch.randn(N, K, h, w, generator=g))
    ws = [rb(torch.randn(C, K, 3, 3, generator=g) * 0.05) for _ in range(4)]
    bs = [torch.randn(C, generator=g) for _ in range(4)]
    gy = rb(torch.randn(N, C, h, w, generator=g))
    xr = x.clone().requires_grad_(True)
    wr = [t.clone().requires_grad_(True) for t in ws]
    y_ref = omodel.aspp_head(xr, wr, bs)
    (y_ref * gy).sum().backward()
    rows = 2 * 4 * C * 9
    zc = (rows + 63) // 64 * 64
    wz = torch.zeros(zc, 1, K)
    for hd, scale in ((0, 1.0), (1, -0.5)):
        for d in range(4):
            wz[(hd * 4 + d) * C * 9:(hd * 4 + d + 1) * C * 9, 0] = (ws[d] * scale).permute(0, 2, 3, 1).reshape(C * 9, K)
    wz = wz.to(BF).to(dev)
    xp = x.permute(0, 2, 3, 1).reshape(N * h * w, K).to(BF).to(dev)
    z = torch.empty(N * h * w, zc, dtype=BF, device=dev)
    ops.conv2d(xp, wz, z, N, h, w, h, w, 1, 1, 1, 0, 1, 0)
    o1, o2 = torch.empty(N, C, h, w, device=dev), torch.empty(N, C, h, w, device=dev)
    ops.aspp_gather(z, [b.to(dev) for b in bs] * 2, o1, o2, N, h, w, C, DIL)
    assert l2(o1, y_ref.detach()) < 1e-2 and l2(o2, omodel.aspp_head(x, [-0.5 * t for t in ws], bs)) < 1e-2
    dz = torch.full((N * h * w, zc), 7.0, dtype=BF, device=dev)
    dbs = [torch.zeros(C, device=dev) for _ in range(8)]
    ops.aspp_scatter(gy.to(dev), torch.zeros(N, C, h, w, device=dev), dz, dbs, N, h, w, C, DIL)
    assert float(dz[:, rows // 2:].abs().max()) == 0.0
    dx = torch.empty(N * h * w, K, dtype=BF, device=dev)
    ops.conv2d(dz, wz.view(zc, K).t().contiguous().view(K, 1, zc), dx, N, h, w, h, w, 1, 1, 1, 0, 1, 0)
    assert l2(dx.float().reshape(N, h, w, K).permute(0, 3, 1, 2), xr.grad) < 1e-2
    gz = torch.zeros(zc, 1, K, device=dev)
    ops.conv2d_wgrad(xp, dz, gz, N, h, w, h, w, 1, 1, 1, 0, 1)
    for d in range(4):
        got = gz[d * C * 9:(d + 1) * C * 9, 0].reshape(C, 3, 3, K).permute(0, 3, 1, 2)
        assert l2(got, wr[d].grad) < 1e-2, d
        np.testing.assert_allclose(dbs[d].cpu().numpy(), gy.sum((0, 2, 3)).numpy(), rtol=1e-4, atol=1e-4)
        assert float(dbs[4 + d].abs().max()) == 0.0


def test_augment_tiles_with_eight_soft_planes():
    """rgda_augment_tiles with the most soft planes it stages (8, the OpenEarthMap / UAVid count): bit for bit against
    tests/aug_ref.py, both pipelines, every geometric element."""
    import random
    import aug_ref
    from regda_amd import ops
    from test_augment_gpu import mag, source
    n, hw, c = 4, 512, 8
    g = torch.Generator().manual_seed(8)
    raw = dict(img=torch.randint(0, 256, (n, hw, hw, 3), generator=g, dtype=torch.uint8),
               label=torch.randint(0, 256, (n, hw, hw), generator=g, dtype=torch.uint8),
               soft=torch.rand(n, c, hw, hw, generator=g),
               regs=torch.randint(0, 1 << 20, (n, hw, hw), generator=g, dtype=torch.int32))
    dev = {k: v.cuda() for k, v in raw.items()}
    rng = random.Random(8)
    for pipe in (mag((256, 256), rng, torch.Generator().manual_seed(8)), source((256, 256), rng, offset=-1, num_class=c)):
        lut, llut = pipe.device_tables('cuda')
        for force in list(range(8)):
            prm = pipe.params(n, hw, hw)
            prm[:, 2] = force
            want = aug_ref.augment(raw['img'], prm, (256, 256), pipe.table(), raw['label'], pipe.label_table(),
                                   raw['soft'], raw['regs'])
            got = ops.augment_tiles(dev['img'], prm, lut, (256, 256), dev['label'], llut, dev['soft'], dev['regs'])
            for k in ('image', 'label', 'soft', 'regs'):
                assert torch.equal(got[k].cpu(), want[k]), (force, k)
