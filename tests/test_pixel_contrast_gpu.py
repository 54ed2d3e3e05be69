"""GPU: rgda_pixel_contrast_select / rgda_pixel_contrast_loss, gast.contrastive.PixelContrastLoss and
AlignStep(contrast_weight=) against the reference's goldens (tests/golden/pixel_contrast.npz), the float64 restatement
and the emulated arithmetic contract (tests/pixel_contrast_ref.py).

Bounds (tests/golden/pixel_contrast_tolerances.json, written by derive_pixel_contrast_tolerances.py, which states the
reasoning): loose = the kernel against float64, 3 x the deviation of the emulated contract from float64, per case;
tight = the kernel against the emulated contract, 3 x the deviation between two summation orders of the emulation plus
the formats' floors (2^-20 loss, 2^-10 gradient).  Against the goldens the reference's own fp32 noise (measured when the
file was minted) is added to the loose bound."""
import json
import os

import pytest
import torch

from pixel_contrast_ref import (NAMES, case_rows, contrast_emulated, contrast_graph, contrast_restated, golden_cases, pixel_rows,
                                production_inputs, production_plan, rows_from_tables, select_restated)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = json.load(open(os.path.join(HERE, 'golden', 'pixel_contrast_tolerances.json')))
REF_NOISE = dict(loss_rel=1.3e-7, grad_rel=2.5e-7)
BF = torch.bfloat16


def _rel(got, ref):
    return ((got.double().cpu() - ref.double()).norm() / ref.double().norm()).item()


@pytest.fixture(scope='module')
def cases(gold):
    return list(golden_cases(gold('pixel_contrast.npz')))


def plan_of(c):
    """the kernel-side plan of a golden case from the recorded draws (no generator involved): anchors, ranks (CPU int32)"""
    from regda_amd.gast.contrastive import plan_anchors
    counts, order, _ = select_restated(c['labels'], c['predict'], 16, tuple(c['feats'].shape[2:]))
    torch.manual_seed(c['seed'])
    anchors, ranks = plan_anchors(counts)
    rows, cls = rows_from_tables(counts, order, anchors, ranks)
    want, _ = case_rows(c)
    assert torch.equal(rows, want)
    return counts, order, anchors, ranks


def run_loss(feats, counts, order, anchors, ranks, dfeat=None, **kw):
    from regda_amd import ops
    return ops.pixel_contrast_loss(feats, order.cuda(), counts.cuda(), anchors.cuda(), ranks.cuda(), dfeat=dfeat, **kw)


def check(name, loss, grows, F, cls, weight=1.0):
    """loss and the gradient at the selected rows against float64 (loose) and the emulated contract (tight)"""
    rl, rg = contrast_restated(F, cls)
    el, eg = contrast_emulated(F, cls, weight=weight)
    l_l, g_l = abs(loss / weight - rl.item()) / abs(rl.item()), _rel(grows / weight, rg)
    l_t, g_t = abs(loss - float(el)) / abs(float(el)), _rel(grows, eg)
    print(name, 'loss', loss, 'float64', rl.item(), 'loose', l_l, g_l, 'tight', l_t, g_t)
    assert l_l <= TOL['bounds'][name]['loss_rel'] and g_l <= TOL['bounds'][name]['grad_rel'], (name, l_l, g_l)
    assert l_t <= TOL['tight'][name]['loss_rel'] and g_t <= TOL['tight'][name]['grad_rel'], (name, l_t, g_t)


def test_select_is_bit_exact_on_the_goldens_labels(cases):
    from regda_amd import ops
    for c in cases:
        size = tuple(c['feats'].shape[2:])
        for C in (7, 16):
            counts, order, flag = ops.pixel_contrast_select(c['labels'].cuda(), c['predict'].cuda(), C, size)
            rc, ro, rf = select_restated(c['labels'], c['predict'], C, size)
            assert torch.equal(counts.cpu(), rc) and torch.equal(order.cpu(), ro) and flag.item() == rf == 0, (c['name'], C)


def test_select_flags_an_out_of_range_label_and_takes_logits_with_ties():
    from regda_amd import ops
    gen = torch.Generator().manual_seed(5)
    labels = torch.randint(-1, 5, (2, 32, 32), generator=gen)
    labels[1, 4, 6] = 9                      # read by the 16 x 16 grid (ratio 2): outside [0, 5), not ignore_label
    labels[0, 3, 3] = 11                     # not read: must not set the flag
    logits = torch.randn(2, 5, 16, 16, generator=gen)
    logits[0, 1, 2, 3] = logits[0, 3, 2, 3] = 7.0          # a planted tie: the lowest index wins
    logits[1, 4, 0, 0] = logits[1, 2, 0, 0] = 9.0
    counts, order, flag = ops.pixel_contrast_select(labels.cuda(), logits.cuda(), 5, (16, 16))
    rc, ro, rf = select_restated(labels, logits, 5, (16, 16))
    assert rf == 4 and flag.item() == 4
    assert torch.equal(counts.cpu(), rc) and torch.equal(order.cpu(), ro)
    pred = ops.argmax_nchw(logits.cuda())
    c2, o2, _ = ops.pixel_contrast_select(labels.cuda(), pred, 5, (16, 16))
    assert torch.equal(c2, counts) and torch.equal(o2, order)
    with pytest.raises(ValueError):
        ops.pixel_contrast_select(labels.cuda(), pred, 5, (16, 16), check=True)
    labels[1, 4, 6] = -1
    assert ops.pixel_contrast_select(labels.cuda(), pred, 5, (16, 16), check=True)[2].item() == 0


def test_loss_and_gradient_match_the_goldens(cases):
    for c in cases:
        counts, order, anchors, ranks = plan_of(c)
        rows, cls = case_rows(c)
        b, k, h, w = c['feats'].shape
        g0 = torch.full((b * h * w, k), 3.0, dtype=BF, device='cuda')
        loss = run_loss(c['feats'].cuda(), counts, order, anchors, ranks, dfeat=g0)
        other = torch.ones(b * h * w, dtype=torch.bool)
        other[rows] = False
        assert not g0.cpu()[other].any(), c['name']                   # accumulate=0: unselected rows are exactly zero
        check(c['name'], loss.item(), g0.cpu()[rows].float(), pixel_rows(c['feats'])[rows], cls)
        lrel, grel = abs(loss.item() - c['loss']) / c['loss'], _rel(g0.cpu()[rows].float(), c['grad'])
        assert lrel <= TOL['bounds'][c['name']]['loss_rel'] + REF_NOISE['loss_rel'], (c['name'], lrel)
        assert grel <= TOL['bounds'][c['name']]['grad_rel'] + REF_NOISE['grad_rel'], (c['name'], grel)
        base = torch.randn(b * h * w, k, generator=torch.Generator().manual_seed(3)).to(BF)
        g1 = base.cuda()
        run_loss(c['feats'].cuda(), counts, order, anchors, ranks, dfeat=g1, accumulate=True)
        assert torch.equal(g1.cpu()[other], base[other]), c['name']    # accumulate=1: unselected rows bit-unchanged
        # the selected rows: bf16(base + fp32 gradient); g0 is that gradient rounded to bf16 (2^-9 relative per element) and
        # the sum is rounded once more (2^-9): per row, 2^-8 of the larger of the two norms
        want, got = base[rows].float() + g0.cpu()[rows].float(), g1.cpu()[rows].float()
        scale = torch.maximum(base[rows].float().norm(dim=1), g0.cpu()[rows].float().norm(dim=1))
        assert ((got - want).norm(dim=1) <= 2.0 ** -8 * scale).all(), c['name']


def test_strided_features_wide_gradient_rows_weight_and_accumulate(cases):
    c = cases[0]
    counts, order, anchors, ranks = plan_of(c)
    rows, cls = case_rows(c)
    b, k, h, w = c['feats'].shape
    big = torch.randn(b + 2, k + 40, h, w, generator=torch.Generator().manual_seed(9)).cuda()
    big[1:1 + b, 8:8 + k] = c['feats'].cuda()
    view = big[1:1 + b, 8:8 + k]                     # channel-sliced and batch-sliced: read in place
    wide = torch.full((b * h * w, k + 24), 5.0, dtype=BF, device='cuda')
    loss = torch.full((1,), 2.0, device='cuda')
    run_loss(view, counts, order, anchors, ranks, dfeat=wide[:, :k], weight=0.25, loss=loss)
    assert (wide[:, k:] == 5.0).all()                # lddf > k: the columns beyond k are not touched
    ref = torch.empty(b * h * w, k, dtype=BF, device='cuda')
    l1 = run_loss(c['feats'].cuda(), counts, order, anchors, ranks, dfeat=ref)
    assert loss.item() == pytest.approx(2.0 + 0.25 * l1.item(), rel=1e-6)      # loss accumulates, scaled by weight
    assert torch.equal(wide[:, :k].float() * 4.0, ref.float())                # a power-of-two weight scales exactly
    twice = ref.clone()
    run_loss(c['feats'].cuda(), counts, order, anchors, ranks, dfeat=twice, accumulate=True)
    assert torch.equal(twice.float(), (2.0 * ref.float()).to(BF).float())
    lo = run_loss(c['feats'].cuda(), counts, order, anchors, ranks)          # loss only
    assert lo.item() == l1.item()


def test_production_channel_count_once():
    from regda_amd import ops
    from regda_amd.gast.contrastive import plan_anchors
    feats, labels, predict, C = production_inputs()
    (rows, cls), perms = production_plan(labels, predict, (32, 32))
    counts, order, flag = ops.pixel_contrast_select(labels.cuda(), predict.cuda(), 16, (32, 32))
    anchors, ranks = plan_anchors(counts.cpu(), generator=torch.Generator().manual_seed(2048))
    got, _ = rows_from_tables(counts.cpu(), order.cpu(), anchors, ranks)
    assert torch.equal(got, rows) and rows.numel() == 800
    g = torch.empty(2 * 1024, 2048, dtype=BF, device='cuda')
    loss = ops.pixel_contrast_loss(feats.cuda(), order, counts, anchors.cuda(), ranks.cuda(), dfeat=g)
    check('production', loss.item(), g.cpu()[rows].float(), pixel_rows(feats)[rows], cls)


def test_two_calls_are_bit_identical(cases):
    c = cases[3]
    counts, order, anchors, ranks = plan_of(c)
    b, k, h, w = c['feats'].shape
    out = []
    for _ in range(2):
        g = torch.empty(b * h * w, k, dtype=BF, device='cuda')
        loss = run_loss(c['feats'].cuda(), counts, order, anchors, ranks, dfeat=g)
        out.append((loss.clone(), g))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_module_reproduces_the_goldens_selection_and_loss(cases):
    from regda_amd.gast.contrastive import PixelContrastLoss
    for c in (cases[0], cases[3], cases[6]):
        rows, cls = case_rows(c)
        leaf = c['feats'].cuda().requires_grad_(True)
        m = PixelContrastLoss()
        torch.manual_seed(c['seed'])                  # seeded like the reference: the reference's draws
        loss = m(leaf, c['labels'].cuda(), c['predict'].cuda())
        (2.0 * loss).backward()
        assert abs(loss.item() - c['loss']) / c['loss'] <= TOL['bounds'][c['name']]['loss_rel'] + REF_NOISE['loss_rel']
        g = pixel_rows(leaf.grad.cpu())               # through autograd into the NCHW leaf
        other = torch.ones(g.shape[0], dtype=torch.bool)
        other[rows] = False
        assert not g[other].any()
        assert _rel(g[rows] / 2.0, c['grad']) <= TOL['bounds'][c['name']]['grad_rel'] + REF_NOISE['grad_rel']
        m2 = PixelContrastLoss(generator=torch.Generator().manual_seed(c['seed']))
        assert m2(c['feats'].cuda(), c['labels'].cuda(), c['predict'].cuda()).item() == loss.item()


def test_module_raises_when_no_class_qualifies(cases):
    from regda_amd.gast.contrastive import PixelContrastLoss
    c = cases[0]
    m = PixelContrastLoss()
    m.max_views = 120                                 # 120 pixels is not more than 120
    with pytest.raises(ValueError, match='no class'):
        m(c['feats'].cuda(), c['labels'].cuda(), c['predict'].cuda())


def _align_step(**kw):
    from oracle import model as omodel
    from regda_amd.align import AlignStep
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.synthetic import make_batch
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, 6, seed=6)
    b = make_batch(b=4, size=128, seed=11, device='cpu')
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(1))
    ones = torch.ones(4, 512)
    m = Deeplabv2(dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True, cascade=False,
                       use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048, num_classes=6,
                       is_ins_norm=True))
    m.load_state_dict(sd, strict=True)
    m.set_drop_masks(ones, ones)
    st = AlignStep(m, protos, **kw)
    g = {k: v.cuda() for k, v in b.items()}
    st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], 1e-3)
    return st, {k: v.detach().clone() for k, v in m.named_parameters()}


def test_align_step_contrast_weight_zero_and_a_batch_without_anchors():
    """On the smallest model shape of tests/test_align_gpu.py (128-pixel tiles: 8 x 8 feature pixels per image) no class
    can have more than 100 pixels, so the term is 0 on both domains: contrast_weight=0 and contrast_weight > 0 both
    give weights bit-identical to a step constructed without the argument, and the step does not raise."""
    _, base = _align_step()
    st0, w0 = _align_step(contrast_weight=0.0)
    st1, w1 = _align_step(contrast_weight=0.5)
    assert st0.loss_contrast.item() == 0.0 and st1.loss_contrast.item() == 0.0
    for k in base:
        assert torch.equal(base[k], w0[k]) and torch.equal(base[k], w1[k]), k


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return (a @ b / (a.norm() * b.norm())).item()


def test_module_reports_a_label_beyond_class_num(cases):
    from regda_amd.gast.contrastive import PixelContrastLoss
    c = cases[0]
    m = PixelContrastLoss(class_num=3)                # the case's labels reach 3
    m(c['feats'].cuda(), c['labels'].cuda(), c['predict'].cuda())
    assert m.last_flag.item() & 4
    m = PixelContrastLoss()
    m(c['feats'].cuda(), c['labels'].cuda(), c['predict'].cuda())
    assert m.last_flag.item() == 0


def test_align_step_contrast_weight_matches_the_composed_oracle(monkeypatch):
    """AlignStep(contrast_weight=w) with a non-zero term on both domains against the composed oracle: the CPU stage-2
    step (oracle.step.CpuAlignStep) plus the restated term (pixel_contrast_ref.contrast_graph on the oracle's own
    features), composed here by wrapping the oracle's two PCL calls as tests/test_whiten_gpu.py does: each adds
    w * PCL_pixel(feat), and the step halves their sum.

    Shape: the smallest the align tests use (2 + 2 tiles of 128^2, 8 x 8 feature pixels per image); max_views is
    lowered to 8 through step.contrast so that classes qualify (n_view = 8).  The step's labels and predictions differ
    from the oracle's in a few borderline pixels (bf16 network), which changes list lengths and with them every
    randperm draw, so the oracle's term is evaluated on the rows the step selected (step.last_contrast); that the
    step selected them from the right inputs is checked separately: its tables equal the restated select on its own
    target label and the source label, with the prediction taken from the ORACLE's logits of the same domain, up to
    5 % of the pixels (the bound test_align_gpu.py grants label_t; swapped source / target logits or labels move
    far more).

    w = 1e-2 makes the term a large share of the gradient (features are unnormalised: the term is about 3e4): the
    oracle's norms with and without it are asserted to differ by >= 1.5, so a missing, halved or doubled gradient moves
    the norm outside the 0.06 of the stage-2 step tests.  The term's own gradient (the flat gradient with the term
    minus the one without, before clipping) is compared with the oracle's difference: cosines > 0.9 and norm within
    0.12, the bounds and reasoning of test_align_step_whiten_weight.  loss_contrast against the restatement on the
    oracle's features, rel 0.05 as for loss_white and loss_domain.  The updated weights: the classifier's update within
    0.08 and the update directions' cosines, as tests/test_align_gpu.py asserts them."""
    from oracle import labelpath, model as omodel
    from oracle.step import CpuAlignStep
    from regda_amd.align import AlignStep
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.synthetic import make_batch
    rt, wt, mv = 'resnet17t', 1e-2, 8
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
        st.contrast['max_views'] = mv
        torch.manual_seed(77)
        out = st.step(gb['images_s'], gb['label_s'], gb['images_t'], gb['regs_t'], 1e-3)
        torch.cuda.synchronize()
        views = {k: m._gviews[k].detach().float().cpu().clone() for k in keys}
        return st, out, m.flat_g.clone(), views, {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    st, (_, _, gn), g_on, v_on, w_on = run_step(contrast_weight=wt)
    _, (_, _, gn_def), g_def, v_def, _ = run_step()
    sel = []
    for side in range(2):
        assert st.last_contrast[side] is not None                          # a non-zero term on both domains
        order, counts, anchors, ranks = (t.cpu() for t in st.last_contrast[side])
        assert ranks.shape[1] == mv and anchors.shape[0] >= 2
        sel.append(rows_from_tables(counts, order, anchors, ranks) + (counts,))

    # the composed oracle: the CPU step, each PCL call + wt * the restated term on the rows the step selected
    pcl, fwd, logits, calls = labelpath.prototype_contrastive_loss, omodel.forward, [], []

    def forward_recording(*a, **k):
        out = fwd(*a, **k)
        logits.append(out[1].detach())
        return out

    def pcl_plus_contrast(prototypes, feat, label, *a, **k):
        rows, cls, _ = sel[len(calls)]
        calls.append(label)
        return pcl(prototypes, feat, label, *a, **k) + wt * contrast_graph(pixel_rows(feat)[rows], cls)

    def oracle():
        return CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, proto_decay=0.999).step(
            b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))
    ref0 = oracle()
    monkeypatch.setattr(omodel, 'forward', forward_recording)
    monkeypatch.setattr(labelpath, 'prototype_contrastive_loss', pcl_plus_contrast)
    cpu = CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, proto_decay=0.999)
    ref = cpu.step(b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))
    monkeypatch.undo()
    assert len(calls) == 2 and len(logits) == 2
    print('oracle: grad norm', ref['grad_norm'], 'without the term', ref0['grad_norm'])
    assert ref['grad_norm'] >= 1.5 * ref0['grad_norm']

    # the step selected from the right inputs: source label with source logits, its target label with target logits
    for side, lab in ((0, b['label_s']), (1, st.last_label_t.cpu())):
        lab = lab.reshape(lab.shape[0], *lab.shape[-2:])
        rc, _, _ = select_restated(lab, logits[side], 6, (8, 8))
        moved = (rc.long() - sel[side][2].long()).abs().sum().item() / 2
        print('side', side, 'pixels in another list than by the oracle\'s logits', moved)
        assert moved <= 0.05 * 128, (side, moved)

    # loss_contrast: the restatement on the oracle's features, the step's rows
    want = wt * 0.5 * sum(contrast_restated(pixel_rows(f)[rows], cls)[0].item() for f, (rows, cls, _) in zip(ref['feats'], sel))
    print('loss_contrast', st.loss_contrast.item(), want, 'grad norm', gn.sqrt().item(), ref['grad_norm'])
    assert want > 0.0 and st.loss_contrast.item() == pytest.approx(want, rel=0.05)
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)
    assert gn_def.sqrt().item() == pytest.approx(ref0['grad_norm'], rel=0.06)

    # the term's own gradient
    ref_delta = {k: ref['grads'][k] - ref0['grads'][k] for k in ref['grads']}
    ref_delta_norm = torch.sqrt(sum((v.double() ** 2).sum() for v in ref_delta.values())).item()
    delta_norm = (g_on.double() - g_def.double()).norm().item()
    print('the term alone', delta_norm, ref_delta_norm)
    assert delta_norm == pytest.approx(ref_delta_norm, rel=0.12)
    for k in keys:
        c = _cos(v_on[k] - v_def[k], ref_delta[k])
        print(k, 'cosine of the term\'s gradient', c)
        assert c > 0.9, (k, c)

    # the updated weights, as tests/test_align_gpu.py asserts them
    for k, tol in (('encoder.resnet.layer4.1.conv3.weight', 0.97), ('encoder.resnet.conv1.weight', 0.9)):
        c = _cos(cpu.sd[k].detach() - sd[k], w_on[k] - sd[k])
        print(k, 'cosine of the update', c)
        assert c > tol, (k, c)
    k = 'layer5.conv_last.4.weight'
    d_ref, d_got = cpu.sd[k].detach() - sd[k], w_on[k] - sd[k]
    assert ((d_got - d_ref).norm() / d_ref.norm()).item() < 0.08
