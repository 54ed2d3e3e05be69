"""GPU: the class-aware whitening loss (rgda_whiten_loss) -- op level against the reference goldens and, at the
production shape, against a CPU emulation of the stated contract and against float64; the drop-in ClassWareWhitening /
Aligner.whiten_class_ware through Deeplabv2's autograd path; AlignStep(whiten_weight=w) against the CPU stage-2 step
composed from the oracle plus the restatement.

Bounds.  Loose (kernel against the reference goldens / against float64 on unrounded features): read from
tests/golden/whiten_tolerances.json, per case 3 x the deviation of the emulated contract from float64 that
tests/golden/derive_whiten_tolerances.py observes on that case's inputs on the CPU.  Tight (kernel against the emulated
contract, where only the order of the fp32 sums differs): loss relative 1e-5, summation-order level: an element of S
is an fp32 sum of n <= 8192 products, reordering moves it by about sqrt(n) 2^-24 = 5e-6 of its size with a random
sign; the sum of the s^2 squares of a block moves by at most sqrt(s^2) 2^-24 = 8e-6 for s = 128 and typically far
less, and the loss averages these independent errors over thousands of elements and up to 192 blocks.  A class mean
that differs in its last bit rounds about 2^-15 sqrt(n) of the centred operands the other way, each 2^-8 of one of
the n products of an element: below 1e-7 of the loss.  1e-5 therefore carries margin and still sees a scaling error
of a single block.  Gradient relative norm 5e-3 (its bf16 store, 2^-9 relative per element = 1.1e-3 RMS, plus the
few elements of bf16(S - I) and of the centred operands that round the other way from a last-bit difference of a
sum).

Every golden case of whiten.npz runs on the kernel.  The hand-worked 6 x 4 example (k = 4, class_ids [1, 2]) is
outside what the kernel serves as stored (4 channels per group; class ids that are not range(C)); it is run embedded
in 32 channels, see test_hand_worked_example_embedded_in_32_channels."""
import json
import os

import numpy as np
import pytest
import torch

from whiten_ref import (golden_cases, production_inputs, rows_of, whiten_differentiable, whiten_emulated,
                        whiten_restated)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = json.load(open(os.path.join(HERE, 'golden', 'whiten_tolerances.json')))['bounds']


def run(feats, labels, C, groups, weight=1.0, **kw):
    """-> (loss tensor, gradient as (b, k, h, w) f32 on the CPU, the raw bf16 rows)"""
    from regda_amd import ops
    b, k, h, w = feats.shape
    rows = torch.empty(b * h * w, k, dtype=BF, device='cuda')
    loss = ops.whiten_loss(feats.cuda(), labels.cuda(), C, groups, -1, weight, dfeat=rows, **kw)
    return loss, rows.float().view(b, h, w, k).permute(0, 3, 1, 2).cpu(), rows


def _rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def test_whiten_loss_matches_every_reference_golden(gold):
    g = gold('whiten.npz')
    cases = list(golden_cases(g))
    assert len(cases) == 3
    for c in cases:
        loss, grad, _ = run(c['feats'], c['labels'], c['class_num'], c['groups'])
        lrel, grel = abs(loss.item() - c['loss']) / c['loss'], _rel(grad, c['grad'])
        print(c['name'], 'loss', loss.item(), c['loss'], 'rel', lrel, 'grad rel', grel)
        el, eg = whiten_emulated(c['feats'], c['labels'], c['class_num'], c['groups'])
        t_l, t_g = abs(loss.item() - el.item()) / el.item(), _rel(grad, eg)
        print(c['name'], 'against the emulated contract: loss rel', t_l, 'grad rel', t_g)
        assert lrel <= TOL[c['name']]['loss_rel'], (c['name'], lrel)
        assert grel <= TOL[c['name']]['grad_rel'], (c['name'], grel)
        assert t_l <= 1e-5 and t_g < 5e-3, (c['name'], t_l, t_g)
        # the rows of ignored pixels and of the singleton class are zeros (accumulate off: every row is written)
        counts = [(c['labels'] == i).sum().item() for i in range(c['class_num'])]
        dead = ((c['labels'] == -1) | (c['labels'] == counts.index(1))).unsqueeze(1).expand_as(grad)
        assert dead.any() and grad[dead].abs().max().item() == 0.0


def test_hand_worked_example_embedded_in_32_channels(gold):
    """The reference's __main__ example has k = 4 channels and class_ids [1, 2]; the kernel serves >= 32 channels per
    group and class_ids = range(C).  Embedded: the four channels padded with 28 zero channels (their covariance rows are
    0, so S - I gains 28 diagonal -1 entries and the mean runs over 32^2 instead of 4^2 elements) and the label 0
    (not in class_ids) mapped to ignore_label: L = (32^2 L_kernel - 28) / 4^2 is the value the reference prints.  The
    inputs are small integers and the class has two pixels, so every operand is exact in bf16."""
    g = gold('whiten.npz')
    feats = torch.zeros(1, 32, 1, 6)
    feats[:, :4] = torch.from_numpy(g['hand_feats'])
    lab = torch.from_numpy(g['hand_lab'].astype(np.int64)).view(1, 1, 6)
    lab = torch.where(lab == 0, torch.full_like(lab, -1), lab)
    loss, grad, _ = run(feats, lab, 6, 1)
    assert (1024.0 * loss.item() - 28.0) / 16.0 == pytest.approx(12.4375, rel=1e-5)
    assert float(g['hand_loss']) == 12.4375
    # gradient: the reference's, rescaled by the 16 / 1024 of the mean (bf16 store)
    want = torch.from_numpy(g['hand_grad']) * (16.0 / 1024.0)
    assert (grad[:, :4] - want).abs().max().item() <= 2 ** -8 * want.abs().max().item()
    assert grad[:, 4:].abs().max().item() == 0.0


def test_whiten_loss_production_shape_against_the_contract_and_fp64():
    """8 x 2048 x 32 x 32, 32 groups of 64 channels, 6 classes of unequal frequency and ignored pixels
    (whiten_ref.production_inputs): tight bounds against the emulated contract, loose (derived) bounds against float64
    on the unrounded features; two runs bit-identical."""
    feats, lab = production_inputs()
    counts = [(lab == i).sum().item() for i in range(6)]
    assert min(counts) >= 2 and max(counts) > 8 * min(counts) and (lab == -1).any()
    loss, grad, rows = run(feats, lab, 6, 32)
    el, eg = whiten_emulated(feats, lab, 6, 32)
    rl, rg = whiten_restated(feats, lab, range(6), 32)
    t_l, t_g = abs(loss.item() - el.item()) / el.item(), _rel(grad, eg)
    l_l, l_g = abs(loss.item() - rl.item()) / rl.item(), _rel(grad, rg)
    print('production: loss', loss.item(), 'emulated', el.item(), 'fp64', rl.item(), 'tight', t_l, t_g, 'loose', l_l, l_g)
    assert t_l <= 1e-5 and t_g < 5e-3
    assert l_l <= TOL['production']['loss_rel'], l_l
    assert l_g <= TOL['production']['grad_rel'], l_g
    loss2, _, rows2 = run(feats, lab, 6, 32)
    assert torch.equal(loss, loss2) and torch.equal(rows, rows2)


def test_whiten_loss_accumulate_weight_zero_rows_and_all_ignored():
    from regda_amd import ops
    gen = torch.Generator().manual_seed(9)
    b, k, h, w, C, groups = 3, 256, 8, 12, 6, 4
    feats = torch.randn(b, k, h, w, generator=gen)
    lab = torch.randint(-1, 4, (b, h, w), generator=gen)
    lab[lab == 3] = -1
    lab[1, 2, 3] = 4                                   # class 4: one pixel; class 5: none
    rl, rg = whiten_restated(feats, lab, range(C), groups)
    loss, grad, rows = run(feats, lab, C, groups)
    assert loss.item() == pytest.approx(whiten_emulated(feats, lab, C, groups)[0].item(), rel=1e-5)
    # accumulate off: the rows of ignored pixels and of the singleton class are written as zeros over what was there
    dirty = torch.full((b * h * w, k), 7.0, dtype=BF, device='cuda')
    ops.whiten_loss(feats.cuda(), lab.cuda(), C, groups, -1, 1.0, dfeat=dirty)
    assert torch.equal(dirty, rows)
    dead = ((lab == -1) | (lab == 4)).reshape(-1)
    assert dead.sum().item() > 10 and rows[dead.cuda()].abs().max().item() == 0.0
    assert (rows[~dead.cuda()].float().abs().amax(1) > 0).all()
    # weight and accumulate onto a non-zero gradient and a non-zero loss
    base = torch.randn(b * h * w, k, generator=gen).mul(rg.abs().max().item()).to(BF).cuda()
    acc = base.clone()
    lacc = torch.full((1,), 2.0, device='cuda')
    ops.whiten_loss(feats.cuda(), lab.cuda(), C, groups, -1, 0.5, loss=lacc, dfeat=acc, accumulate=True)
    assert lacc.item() == pytest.approx(2.0 + 0.5 * loss.item(), rel=1e-6)
    want = base.double().cpu() + 0.5 * rows_of(rg)
    err = (acc.double().cpu() - want).abs()
    # fp32 add, one bf16 rounding of the sum: |err| <= 2^-8 |sum| per element, plus the gradient's own error
    assert (err <= 2 ** -8 * want.abs() + 1e-2 * rg.abs().max().item()).all()
    assert torch.equal(acc[dead.cuda()], base[dead.cuda()])          # untouched rows
    # every label ignored: loss 0, zero gradient
    none = torch.full((b, h, w), -1, dtype=torch.long)
    l0, g0, _ = run(feats, none, C, groups)
    assert l0.item() == 0.0 and g0.abs().max().item() == 0.0
    # the loss alone (no gradient buffer)
    assert torch.equal(ops.whiten_loss(feats.cuda(), lab.cuda(), C, groups), loss)
    # a channel and batch slice of a larger map is read in place through its strides: the same bits
    big = torch.randn(b + 1, k + 96, h, w, generator=gen).cuda()
    big[1:, 32:32 + k] = feats.cuda()
    view = big[1:, 32:32 + k]
    assert not view.is_contiguous()
    sliced = torch.full((b * h * w, k), 7.0, dtype=BF, device='cuda')
    assert torch.equal(ops.whiten_loss(view, lab.cuda(), C, groups, -1, 1.0, dfeat=sliced), loss)
    assert torch.equal(sliced, rows)


@pytest.mark.parametrize('C', [7, 16])
@pytest.mark.parametrize('k,groups', [(64, 2), (192, 2), (256, 2)])
def test_whiten_loss_class_counts_and_block_sizes(C, k, groups):
    """7 and 16 classes; 32, 96 and 128 channels per group (64 is the production test's), against the emulated
    contract with the tight bounds (the derived loose bounds belong to the inputs they were derived on)"""
    gen = torch.Generator().manual_seed(100 * C + k)
    feats = torch.randn(2, k, 16, 20, generator=gen) * 1.3
    lab = torch.randint(-1, C, (2, 16, 20), generator=gen)
    loss, grad, _ = run(feats, lab, C, groups)
    el, eg = whiten_emulated(feats, lab, C, groups)
    t_l, t_g = abs(loss.item() - el.item()) / el.item(), _rel(grad, eg)
    print('C', C, 'k', k, 'groups', groups, 'against the emulated contract: loss rel', t_l, 'grad rel', t_g)
    assert t_l <= 1e-5 and t_g < 5e-3


def test_whiten_loss_flags_labels_out_of_range():
    from regda_amd import ops
    gen = torch.Generator().manual_seed(3)
    feats = torch.randn(1, 64, 8, 8, generator=gen)
    lab = torch.randint(0, 6, (1, 8, 8), generator=gen)
    _, ws = ops.whiten_loss(feats.cuda(), lab.cuda(), 6, 1, -1, return_ws=True)
    words = ws[:68].view(torch.int32).cpu()
    assert words[0].item() == 0
    assert words[1:7].tolist() == [(lab == i).sum().item() for i in range(6)]
    bad = lab.clone()
    bad[0, 0, 0] = 6
    bad[0, 0, 1] = -2
    lb, ws = ops.whiten_loss(feats.cuda(), bad.cuda(), 6, 1, -1, return_ws=True)
    assert ws[:4].view(torch.int32).item() & 4
    with pytest.raises(ValueError):
        ops.whiten_loss(feats.cuda(), bad.cuda(), 6, 1, -1, check=True)
    # the out-of-range pixels count as ignored
    ign = torch.where((bad < 0) | (bad > 5), torch.full_like(bad, -1), bad)
    assert torch.equal(lb, ops.whiten_loss(feats.cuda(), ign.cuda(), 6, 1, -1))
    with pytest.raises(ValueError):
        ops.whiten_loss(torch.randn(1, 2048, 4, 4).cuda(), torch.zeros(1, 4, 4, dtype=torch.long).cuda(), 6, 1)


# ------------------------------------------------------------------------------------------- module and step
def _model(rt, sd):
    from regda_amd.models.Encoder import Deeplabv2
    m = Deeplabv2(dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True, cascade=False,
                       use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048, num_classes=6,
                       is_ins_norm=True))
    m.load_state_dict(sd, strict=True)
    return m


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return (a @ b / (a.norm() * b.norm())).item()


def _blocky_labels(seed, b=2, size=128, C=6):
    """full-size labels in 16 x 16 blocks (so the 16x downscale keeps them), a few blocks ignored"""
    gen = torch.Generator().manual_seed(seed)
    cells = torch.randint(-1, 3, (b, size // 16, size // 16), generator=gen)
    return cells.repeat_interleave(16, 1).repeat_interleave(16, 2).long()


@pytest.mark.parametrize('with_target', [False, True])
def test_aligner_whiten_class_ware_through_the_model_autograd_path(with_target):
    """model(xs) [, model(xt)], aligner.whiten_class_ware(...), loss.backward(): the loss against the emulated
    contract on the GPU model's own features (tight bound) and against the CPU oracle's composition (rel 0.05, as for
    CORAL: bf16 network against fp32); parameter gradients against the CPU oracle's
    autograd of the same composition (cosines, as for CORAL: bf16 network against fp32)."""
    from oracle import labels as olab, model as omodel
    from regda_amd.gast.alignment import Aligner
    from regda_amd.gast.class_ware_whiten import ClassWareWhitening
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, 6, seed=21)
    gen = torch.Generator().manual_seed(3)
    xs, xt = torch.randn(2, 3, 128, 128, generator=gen), torch.randn(2, 3, 128, 128, generator=gen) * 1.3
    ls, lt = _blocky_labels(5), _blocky_labels(6)
    down = lambda l: torch.from_numpy(olab.downscale_label(l.numpy(), 16, 6, -1, 0.75))      # noqa: E731
    # CPU oracle
    w = {k: v.clone() for k, v in sd.items()}
    names = omodel.param_names(w)
    for k in names:
        w[k].requires_grad_(True)
    _, _, fs = omodel.forward(w, xs, True, None, rt, {})
    ref = whiten_differentiable(fs, down(ls), range(6), 32)
    if with_target:
        _, _, ft = omodel.forward(w, xt, True, None, rt, {})
        ref = 0.5 * (ref + whiten_differentiable(ft, down(lt), range(6), 32))
    grads = dict(zip(names, torch.autograd.grad(ref, [w[k] for k in names], allow_unused=True)))
    # the library
    m = _model(rt, sd)
    m.train()
    al = Aligner(None, feat_channels=2048, class_num=6)
    assert isinstance(al.whitener, ClassWareWhitening) and al.whitener.groups == 32
    _, _, gfs = m(xs.cuda())
    if with_target:
        _, _, gft = m(xt.cuda())
        loss = al.whiten_class_ware(gfs, ls.cuda(), gft, lt.cuda())
        own = 0.5 * (whiten_emulated(gfs.detach().cpu(), down(ls), 6, 32)[0] +
                     whiten_emulated(gft.detach().cpu(), down(lt), 6, 32)[0])
    else:
        loss = al.whiten_class_ware(gfs, ls.cuda())
        own = whiten_emulated(gfs.detach().cpu(), down(ls), 6, 32)[0]
    loss.backward()
    print('whiten_class_ware', with_target, loss.item(), own.item(), ref.item())
    assert loss.item() == pytest.approx(own.item(), rel=1e-5)
    assert loss.item() == pytest.approx(ref.item(), rel=0.05)
    named = dict(m.named_parameters())
    for k in ('encoder.resnet.layer4.1.conv3.weight', 'encoder.resnet.layer1.0.conv1.weight', 'encoder.resnet.conv1.weight'):
        c = _cos(named[k].grad.cpu(), grads[k])
        assert c > 0.9, (k, c)
    # the classifier heads do not see the whitening loss
    assert named['layer5.conv_last.4.weight'].grad.abs().max().item() == 0.0


def test_align_step_whiten_weight(monkeypatch):
    """AlignStep(whiten_weight=w) against the CPU stage-2 step with the term added (the oracle's PCL calls are wrapped:
    each adds w * W(feat, label), and the step halves their sum).

    w = 2 makes the term a large share of the gradient: the oracle's own two steps (with and without the term) are
    asserted to differ by a factor >= 1.5 in gradient norm (1.70 on the CPU; the term's gradient is nearly orthogonal
    to the rest, 81.5 w against 119.3), so a missing, halved (1.21) or doubled (2.9) whitening gradient moves the norm
    far outside the 0.06 of the other stage-2 step tests.  A norm cannot see a sign or a gradient written onto the
    wrong half of gfeat, so the term's own gradient -- the step's flat gradient with the term minus the one without,
    both before clipping -- is compared with the oracle's difference: per-tensor cosines > 0.9 (as for CORAL: bf16
    network against fp32) and its norm within 0.12: each of the two gradients carries the bf16 network's deviation,
    the 0.06 granted to its norm, and the difference of norm 1.37 |g0| is taken from gradients of norm |g0| and
    1.70 |g0| (the oracle's figures): 0.06 * (1 + 1.70) / 1.37 = 0.12.
    loss_white (the term as it enters the loss, w * 0.5 * (W_s + W_t)) against the restatement on the oracle's forward
    features with the step's own downscaled labels, rel 0.05 as for loss_domain; whiten_weight=0.0 leaves the weights
    bit-identical to a step built without the argument; two runs bit-identical."""
    from oracle import labelpath, model as omodel
    from oracle.step import CpuAlignStep
    from regda_amd.align import AlignStep
    from regda_amd.synthetic import make_batch
    rt, wt = 'resnet17t', 2.0
    sd = omodel.init_state_dict(rt, 6, seed=6)
    b = make_batch(b=2, size=128, seed=11, device='cpu')
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(1))
    ones = torch.ones(2, 512)
    pcl = labelpath.prototype_contrastive_loss

    def oracle():
        return CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, proto_decay=0.999).step(
            b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))

    def pcl_plus_whitening(prototypes, feat, label, *a, **k):
        return pcl(prototypes, feat, label, *a, **k) + wt * whiten_differentiable(feat, label, range(6), 32)
    ref0 = oracle()
    monkeypatch.setattr(labelpath, 'prototype_contrastive_loss', pcl_plus_whitening)
    ref = oracle()
    monkeypatch.undo()
    ref_delta = {k: ref['grads'][k] - ref0['grads'][k] for k in ref['grads']}
    ref_delta_norm = torch.sqrt(sum((v.double() ** 2).sum() for v in ref_delta.values())).item()
    print('oracle: grad norm', ref['grad_norm'], 'without the term', ref0['grad_norm'], 'the term alone', ref_delta_norm)
    assert ref['grad_norm'] >= 1.5 * ref0['grad_norm']
    gb = {k: v.cuda() for k, v in b.items()}
    keys = ('encoder.resnet.layer4.1.conv3.weight', 'encoder.resnet.layer1.0.conv1.weight', 'encoder.resnet.conv1.weight')

    def make(**kw):
        m = _model(rt, sd)
        m.set_drop_masks(ones, ones)
        return AlignStep(m, protos, **kw)

    def weights_after(**kw):
        """-> step, its outputs, the weights after it, the flat gradient (before clipping), its views of `keys`"""
        st = make(**kw)
        out = st.step(gb['images_s'], gb['label_s'], gb['images_t'], gb['regs_t'], 1e-3)
        torch.cuda.synchronize()
        views = {k: st.model._gviews[k].detach().float().cpu().clone() for k in keys}
        return st, out, st.model.flat_p.clone(), st.model.flat_g.clone(), views
    st, (ls, la, gn), w_on, g_on, v_on = weights_after(whiten_weight=wt)
    fs, ft = ref['feats']
    want = wt * 0.5 * (whiten_restated(fs, st.last_label_s_down.cpu(), range(6), 32)[0] +
                       whiten_restated(ft, st.last_label_t.cpu(), range(6), 32)[0]).item()
    print('align step: loss_white', st.loss_white.item(), want, 'grad norm', gn.sqrt().item(), ref['grad_norm'],
          'loss_align', la.item(), ref['loss_align'])
    assert want > 0.0 and st.loss_white.item() == pytest.approx(want, rel=0.05)
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)
    assert g_on.double().norm().item() == pytest.approx(gn.sqrt().item(), rel=1e-5)      # flat_g is the unclipped gradient
    _, _, w_on2, g_on2, _ = weights_after(whiten_weight=wt)
    assert torch.equal(w_on, w_on2) and torch.equal(g_on, g_on2)
    st0, _, w_zero, _, _ = weights_after(whiten_weight=0.0)
    _, (_, _, gn_def), w_def, g_def, v_def = weights_after()
    assert torch.equal(w_zero, w_def) and not torch.equal(w_on, w_def)
    assert st0.loss_white.item() == 0.0
    assert gn_def.sqrt().item() == pytest.approx(ref0['grad_norm'], rel=0.06)
    # the term's own gradient
    delta_norm = (g_on.double() - g_def.double()).norm().item()
    print('grad norm without the term', gn_def.sqrt().item(), ref0['grad_norm'], 'the term alone', delta_norm, ref_delta_norm)
    assert delta_norm == pytest.approx(ref_delta_norm, rel=0.12)
    for k in keys:
        c = _cos(v_on[k] - v_def[k], ref_delta[k])
        print(k, 'cosine of the term\'s gradient', c)
        assert c > 0.9, (k, c)
    with pytest.raises(ValueError):
        make(whiten_weight=-1.0)
