"""GPU: the semantic-aware whitening loss (rgda_saw_loss) -- op level against the reference goldens, against the float64
restatement at edge shapes and at the production shape; the drop-in SAW module; AlignStep(saw_weight=w) against the CPU
stage-2 step composed from the oracle plus the restatement.

Near ties are a condition, not a tolerance.  The sign of a pair covariance and the active bit of a group are decisions;
the kernel's (read from its table, ops.saw_tables) may differ from float64's only inside a guard band: |corr| <
2 hw 2^-24 for a pair (an fp32 dot product of hw terms errs by at most hw 2^-24 |a| |b|, doubled), and nod times that on
s - margin for a group.  Outside the bands the table equals the float64 one exactly; inside, at most 0.1 % of all pairs
and 0.1 % of all groups may differ.  The gradient is then compared with the float64 formula evaluated on the kernel's
table.

Bounds.  Loss against the reference goldens / float64 at the production shape: tests/golden/saw_tolerances.json, per case
3 x the deviation of an fp32 evaluation of the contract from float64 (tests/golden/derive_saw_tolerances.py), relative
to sum over the active groups of s / (nod B).  Loss at the edge shapes, which have no derived figure: the worst case of
the fp32 sums, saw_ref.fp32_loss_bound.  Gradient: relative norm within the derived bound plus 5e-3, the project's figure
for a bf16-stored gradient (2^-9 per element is 1.1e-3 RMS)."""
import json
import os

import pytest
import torch

from saw_ref import (fp32_loss_bound, fp32_s_bound, golden_cases, group_band, loss_scale, pair_band, production_inputs, saw_differentiable,
                     saw_plan, saw_restated)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = json.load(open(os.path.join(HERE, 'golden', 'saw_tolerances.json')))['bounds']
BF16_GRAD = 5e-3


def _rel(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def _as_map(rows, shape):
    b, k, h, w = shape
    return rows.float().view(b, h, w, k).permute(0, 3, 1, 2).cpu()


def run(feats, W, sel, relax, weight=1.0, fill=7.0, **kw):
    """-> (loss tensor, gradient as (b, k, h, w) f32 on the CPU, the bf16 rows (a view of a buffer whose rows are padded to
    a multiple of 8 columns), the padded buffer, the kernel's tables)"""
    from regda_amd import ops
    b, k, h, w = feats.shape
    buf = torch.full((b * h * w, (k + 7) // 8 * 8), fill, dtype=BF, device='cuda')
    rows = buf[:, :k]
    loss, ws = ops.saw_loss(feats.cuda(), W.cuda(), sel, relax, weight, dfeat=rows, return_ws=True, **kw)
    tab = {n: (v.cpu() if torch.is_tensor(v) else v) for n, v in ops.saw_tables(ws, b, k, len(sel)).items()}
    return loss, _as_map(rows, feats.shape), rows, buf, tab


def tie_condition(tab, r, hw, C, who):
    """the kernel's decisions against float64's `r`: equal outside the guard bands, at most 0.1 % differ inside"""
    dp = tab['signs'] != r['signs']
    dg = tab['active'] != r['active']
    in_p = r['corr'].abs() < pair_band(hw)
    in_g = (r['s'] - r['margin']).abs() < group_band(hw, C)
    print(who, 'pairs', dp.numel(), 'in the band', int(in_p.sum()), 'differ', int(dp.sum()), '| groups', dg.numel(), 'in the band',
          int(in_g.sum()), 'differ', int(dg.sum()))
    assert not (dp & ~in_p).any(), who
    assert not (dg & ~in_g).any(), who
    assert int(dp.sum()) <= 1e-3 * dp.numel() and int(dg.sum()) <= 1e-3 * dg.numel(), who
    assert in_p.sum().item() <= 1e-3 * dp.numel() and in_g.sum().item() <= 1e-3 * dg.numel(), who      # the inputs' own share


def check(feats, W, sel, relax, who, loss_bound=None, grad_bound=BF16_GRAD):
    """the kernel on these inputs against float64: the plan tables, the tie condition, the loss (absolute bound; the fp32
    worst case by default), the gradient on the kernel's own table.  -> (loss, grad, rows, buf, tab, float64 result)"""
    b, k, h, w = feats.shape
    C, hw = len(sel), h * w
    loss, grad, rows, buf, tab = run(feats, W, sel, relax)
    r = saw_restated(feats, W, sel, relax)
    assert tab['flag'] == 0
    assert torch.equal(tab['ch'].long(), r['ch']), who
    assert (tab['wgh'].double() - r['wgh']).abs().max().item() <= 2.0 ** -24, who          # sigmoid < 1, rounded once
    inv = torch.full((k, C), -1, dtype=torch.int32)
    for j in range(C):
        inv[r['ch'][:, j], j] = torch.arange(r['ch'].shape[0], dtype=torch.int32)
    assert torch.equal(tab['inv'], inv), who
    tie_condition(tab, r, hw, C, who)
    assert ((tab['s'].double() - r['s']).abs() <= fp32_s_bound(r, hw)).all(), who
    bound = fp32_loss_bound(r, hw) if loss_bound is None else loss_bound(r)
    print(who, 'loss', loss.item(), 'float64', r['loss'].item(), 'deviation', abs(loss.item() - r['loss'].item()), 'bound', bound)
    assert abs(loss.item() - r['loss'].item()) <= bound, who
    on_table = saw_restated(feats, W, sel, relax, table=dict(signs=tab['signs'], active=tab['active']))
    if on_table['grad'].abs().max().item() > 0:
        g = _rel(grad, on_table['grad'])
        print(who, 'gradient relative norm', g, 'bound', grad_bound)
        assert g <= grad_bound, who
    else:
        assert grad.abs().max().item() == 0.0
    if buf.shape[1] > k:
        assert (buf[:, k:] == 7.0).all(), who               # the padding columns of a row are not written
    return loss, grad, rows, buf, tab, r


# ------------------------------------------------------------------------------------------- goldens
def test_saw_loss_matches_every_reference_golden(gold):
    cases = list(golden_cases(gold('saw.npz')))
    assert [c['name'] for c in cases] == ['k64_c6', 'k70_c8', 'k48_c16', 'k32_c2', 'k32_c4_sel', 'hw2']
    for c in cases:
        b, k, h, w = c['feats'].shape
        tol = TOL[c['name']]
        loss, grad, rows, buf, tab, r = check(c['feats'], c['W'], c['selected'], c['relax_denom'], c['name'],
                                              grad_bound=tol['grad_rel'] + BF16_GRAD)
        assert torch.equal(tab['signs'], r['signs']) and torch.equal(tab['active'], r['active'])      # minted without near ties
        scale = loss_scale(r)
        lrel, grel = abs(loss.item() - c['loss']) / scale, _rel(grad, c['grad'])
        print(c['name'], 'loss', loss.item(), 'reference', c['loss'], 'deviation / scale', lrel, 'bound', tol['loss_rel'],
              'grad rel', grel)
        assert lrel <= tol['loss_rel'], (c['name'], lrel)
        assert grel <= tol['grad_rel'] + BF16_GRAD, (c['name'], grel)
        free = torch.ones(k, dtype=torch.bool)
        free[r['ch'].reshape(-1)] = False
        assert free.any() and grad[:, free].abs().max().item() == 0.0       # channels that fill no slot read exactly 0


# ------------------------------------------------------------------------------------------- edges
def _edge_inputs(seed, b=2, k=40, h=5, w=13, n_cls=6, scale=2.0):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(b, 2, h, w, generator=gen)
    feats = (torch.randn(b, k, h, w, generator=gen) + torch.einsum('kr,brhw->bkhw', torch.randn(k, 2, generator=gen), z)) * scale
    return feats, torch.randn(n_cls, k, generator=gen), gen


def test_two_classes_share_their_rank_0_channel():
    """a duplicate inside a group: the same plane twice, their covariance is its (positive) squared norm"""
    feats, W, _ = _edge_inputs(11)
    W[1, 17] = 7.0
    W[4, 17] = -8.0
    sel = list(range(6))
    ch, _ = saw_plan(W, sel)
    assert ch[0, 1] == 17 and ch[0, 4] == 17
    _, grad, _, _, tab, r = check(feats, W, sel, 2.0, 'shared rank 0')
    assert r['active'][:, 0].all() and grad[:, 17].abs().max().item() > 0


def test_one_channel_fills_a_slot_of_every_class():
    """channel 5 has rank j for class j: C slots in C different groups, gathered in class order"""
    feats, W, _ = _edge_inputs(12, k=44)
    sel = list(range(6))
    for j in sel:
        v = torch.cat([W[j, :5], W[j, 6:]]).abs().sort(descending=True).values
        W[j, 5] = v[0] + 1.0 if j == 0 else 0.5 * (v[j - 1] + v[j])
    ch, _ = saw_plan(W, sel)
    assert [int(ch[j, j]) for j in sel] == [5] * 6
    _, grad, _, _, tab, r = check(feats, W, sel, 0, 'one channel, six slots')
    assert (tab['inv'][5] == torch.arange(6, dtype=torch.int32)).all()
    # and all six slots of one group: the group is the channel six times over
    W[:, 9] = torch.tensor([20.0, -21.0, 22.0, -23.0, 24.0, 25.0])
    ch, _ = saw_plan(W, sel)
    assert (ch[0] == 9).all()
    check(feats, W, sel, 0, 'one channel, one whole group')


def test_equal_weights_rank_by_the_lower_channel_index():
    feats, W, _ = _edge_inputs(13, k=48, n_cls=4)
    W[0, 8:20] = 1.25                                     # a run of equal |w| inside the used ranks, signs mixed
    W[0, 8:20:2] *= -1
    W[1, :] = 0.75                                        # a whole class of equal |w|: rank = channel index
    W[2, 30:48] = 0.0                                     # a run of zeros at the unused end
    W[3, 40] = W[3, 3] = 3.5                              # two equal maxima
    sel = [0, 1, 2, 3]
    _, _, _, _, tab, r = check(feats, W, sel, 0, 'ties')
    assert tab['ch'][:, 1].tolist() == list(range(12))
    assert tab['ch'][0, 3].item() == 3 and tab['ch'][1, 3].item() == 40
    order0 = tab['ch'][:, 0].tolist()
    tied = [c for c in order0 if 8 <= c < 20]
    assert tied == sorted(tied) and len(tied) >= 2


def test_margin_above_every_group_gives_exactly_zero():
    """relax_denom 1.0: margin = nod = 15, and every s of these small features is far below: the loss is exactly 0 and
    every row is written as zeros over a dirty buffer"""
    feats, W, _ = _edge_inputs(14, scale=0.2)
    loss, grad, rows, buf, tab, r = check(feats, W, list(range(6)), 1.0, 'all clamped')
    assert r['margin'] == 15.0 and 0.0 < r['s'].max().item() < 0.5 * r['margin'] and not tab['active'].any()
    assert loss.item() == 0.0 and (rows == 0).all()


def test_accumulate_weight_loss_alone_and_views():
    from regda_amd import ops
    feats, W, gen = _edge_inputs(15, b=3, k=64, h=6, w=11, scale=0.6)
    b, k, h, w = feats.shape
    sel, relax = list(range(6)), 4.0                       # margin 3: some groups active, some clamped
    loss, grad, rows, buf, tab, r = check(feats, W, sel, relax, 'accumulate base')
    assert r['active'].any() and (~r['active']).any()
    rg = saw_restated(feats, W, sel, relax, table=dict(signs=tab['signs'], active=tab['active']))['grad']
    rows_ref = rg.permute(0, 2, 3, 1).reshape(-1, k)
    # weight and accumulate onto a non-zero gradient and a non-zero loss
    base = torch.randn(b * h * w, k, generator=gen).mul(rg.abs().max().item()).to(BF).cuda()
    acc = base.clone()
    lacc = torch.full((1,), 2.0, device='cuda')
    ops.saw_loss(feats.cuda(), W.cuda(), sel, relax, 0.5, loss=lacc, dfeat=acc, accumulate=True)
    assert lacc.item() == pytest.approx(2.0 + 0.5 * loss.item(), rel=1e-6)
    want = base.double().cpu() + 0.5 * rows_ref
    err = (acc.double().cpu() - want).abs()
    # fp32 add, one bf16 rounding of the sum: |err| <= 2^-8 |sum| per element, plus the gradient's own error
    assert (err <= 2 ** -8 * want.abs() + 1e-2 * rg.abs().max().item()).all()
    # untouched under accumulate: the channels that fill no slot, and per image those whose groups are all inactive
    touched = torch.zeros(b, k, dtype=torch.bool)
    for g in range(r['ch'].shape[0]):
        for j in range(6):
            touched[:, r['ch'][g, j]] |= tab['active'][:, g]
    free = ~touched.any(0)
    assert free.any() and (~touched).sum() > free.sum() * b
    same = (acc == base).cpu().view(b, h * w, k)
    assert same.permute(0, 2, 1)[~touched].all()
    assert (rows.cpu().view(b, h * w, k).permute(0, 2, 1)[~touched] == 0).all()          # and zeros without accumulate
    # the loss alone (no gradient buffer; the workspace may omit the slot gradients)
    assert torch.equal(ops.saw_loss(feats.cuda(), W.cuda(), sel, relax), loss)
    # a channel and batch slice of a larger map is read in place through its strides: the same bits
    big = torch.randn(b + 1, k + 24, h, w, generator=gen).cuda()
    big[1:, 16:16 + k] = feats.cuda()
    view = big[1:, 16:16 + k]
    assert not view.is_contiguous()
    sliced = torch.full((b * h * w, k), 7.0, dtype=BF, device='cuda')
    assert torch.equal(ops.saw_loss(view, W.cuda(), sel, relax, 1.0, dfeat=sliced), loss)
    assert torch.equal(sliced, rows)
    # a row slice of a larger classifier, read through its row stride
    wide = torch.randn(6, k + 8, generator=gen).cuda()
    wide[:, :k] = W.cuda()
    again = torch.full((b * h * w, k), 7.0, dtype=BF, device='cuda')
    assert torch.equal(ops.saw_loss(feats.cuda(), wide[:, :k], sel, relax, 1.0, dfeat=again), loss)
    assert torch.equal(again, rows)


def test_non_finite_weight_sets_the_flag():
    from regda_amd import ops
    feats, W, _ = _edge_inputs(16)
    sel = list(range(6))
    _, ws = ops.saw_loss(feats.cuda(), W.cuda(), sel, 2.0, return_ws=True)
    assert ops.saw_tables(ws, 2, 40, 6)['flag'] == 0
    for bad in (float('nan'), float('inf')):
        Wb = W.clone()
        Wb[2, 7] = bad
        rows = torch.empty(2 * 5 * 13, 40, dtype=BF, device='cuda')
        _, ws = ops.saw_loss(feats.cuda(), Wb.cuda(), sel, 2.0, dfeat=rows, return_ws=True)
        torch.cuda.synchronize()
        tab = ops.saw_tables(ws, 2, 40, 6)
        assert tab['flag'] & 1
        assert int(tab['ch'].min()) >= 0 and int(tab['ch'].max()) < 40         # the plan is still a plan
        with pytest.raises(ValueError, match='not finite'):
            ops.saw_loss(feats.cuda(), Wb.cuda(), sel, 2.0, check=True)
    Wb = W.clone()
    Wb[5, 7] = float('nan')                                # a class that is not selected is not read
    _, ws = ops.saw_loss(feats.cuda(), Wb.cuda(), [0, 1, 2, 3], 2.0, return_ws=True)
    assert ops.saw_tables(ws, 2, 40, 4)['flag'] == 0
    with pytest.raises(ValueError):
        ops.saw_loss(feats.cuda(), W.cuda(), [0, 1, 2], 2.0)
    with pytest.raises(ValueError):
        ops.saw_loss(feats.cuda(), W.cuda(), [0, 1, 2, 2], 2.0)


@pytest.mark.parametrize('C,k,h,w', [(2, 9, 3, 3), (4, 130, 17, 19), (8, 72, 9, 31), (16, 100, 16, 17)])
def test_class_counts_odd_sizes_and_several_tiles(C, k, h, w):
    """every served class count next to k and hw that are no multiple of the 64 x 64 gradient tile or of 4 channels, more
    than 256 pixels (several strides of the dot products) and fewer than 64"""
    gen = torch.Generator().manual_seed(100 * C + k)
    feats = torch.randn(2, k, h, w, generator=gen) + 2.5 * torch.randn(2, 1, h, w, generator=gen)
    W = torch.randn(C + 1, k, generator=gen)
    sel = list(range(1, C + 1))
    nod = C * (C - 1) // 2
    _, _, _, _, tab, r = check(feats, W, sel, 0 if C == 2 else nod / (0.6 * nod), f'C {C} k {k} hw {h * w}')
    assert r['active'].any()


# ------------------------------------------------------------------------------------------- production shape
def test_saw_loss_production_shape():
    """8 x 2048 x 32 x 32, 6 classes, relax_denom 2.0 (saw_ref.production_inputs): the derived bounds against float64, the
    tie condition, two runs bit-identical"""
    feats, W = production_inputs()
    sel = list(range(6))
    tol = TOL['production']
    loss, grad, rows, buf, tab, r = check(feats, W, sel, 2.0, 'production', loss_bound=lambda r: tol['loss_rel'] * loss_scale(r),
                                          grad_bound=tol['grad_rel'] + BF16_GRAD)
    assert 0.05 < r['active'].float().mean().item() < 0.95
    loss2, _, rows2, _, tab2 = run(feats, W, sel, 2.0)
    assert torch.equal(loss, loss2) and torch.equal(rows, rows2)
    assert torch.equal(tab['signs'], tab2['signs']) and torch.equal(tab['active'], tab2['active'])


# ------------------------------------------------------------------------------------------- module and step
def test_saw_module_is_the_reference_signature():
    from regda_amd.gast.SAW import SAW
    gen = torch.Generator().manual_seed(8)
    k, n_cls, sel = 64, 7, [1, 2, 4, 6]
    torch.manual_seed(8)
    conv = torch.nn.Conv2d(k, n_cls, 1).cuda()      # default initialisation: |w| <= 1 / 8, every sigmoid near 0.5
    x = (torch.randn(2, k, 6, 10, generator=gen) + 3.0 * torch.randn(2, 1, 6, 10, generator=gen)).cuda().requires_grad_(True)
    crit = SAW(conv, sel, relax_denom=3.0)
    loss = crit(x)
    assert loss.shape == (1,) and loss.requires_grad
    (2.0 * loss).sum().backward()
    W = conv.weight.detach().squeeze().cpu()
    r = saw_restated(x.detach().cpu(), W, sel, 3.0)
    assert r['active'].any()
    assert abs(loss.item() - r['loss'].item()) <= fp32_loss_bound(r, 60)
    assert _rel(x.grad.cpu(), 2.0 * r['grad']) <= BF16_GRAD
    assert conv.weight.grad is None and conv.bias.grad is None          # differentiable to x only
    # a tensor in place of the module (an extension)
    x2 = x.detach().clone().requires_grad_(True)
    loss2 = SAW(W.cuda(), sel, relax_denom=3.0)(x2)
    assert torch.equal(loss2, loss)
    with pytest.raises(ValueError):
        SAW(conv, [0, 1, 2])


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


def test_align_step_saw_weight(monkeypatch):
    """AlignStep(saw_weight=w) against the CPU stage-2 step with the term added (the oracle's PCL calls are wrapped: each
    adds w * SAW(feat; the prototypes PCL is given, relax_denom 0), and the step halves their sum).

    w = 3 makes the term a large share of the gradient: on the CPU the oracle's gradient norm is 119.34 without the term
    and 213.83 with it (a factor 1.79, asserted >= 1.5; 1.12 at w = 1); the term's own gradient, the difference of the
    two, has norm 174.24 (58.08 w).  That difference is compared with the step's (flat gradient with the term minus
    without it, both before clipping): per-tensor cosines > 0.9, and its norm within 0.06 (|g0| + |g1|) / |delta| =
    0.06 * (119.34 + 213.83) / 174.24 = 0.115: each of the two gradients carries the bf16 network's deviation, the 0.06
    granted to its norm.
    loss_saw (the term as it enters the loss, w * 0.5 * (SAW_s + SAW_t)) against the restatement on the oracle's forward
    features and the step's prototypes, rel 0.05 as for the other terms; saw_weight=0.0 leaves the weights bit-identical
    to a step built without the argument; two runs bit-identical; a caller's classifier tensor changes the result."""
    from oracle import labelpath, model as omodel
    from oracle.step import CpuAlignStep
    from regda_amd.align import AlignStep
    from regda_amd.synthetic import make_batch
    rt, wt = 'resnet17t', 3.0
    sel = list(range(6))
    sd = omodel.init_state_dict(rt, 6, seed=6)
    b = make_batch(b=2, size=128, seed=11, device='cpu')
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(1))
    ones = torch.ones(2, 512)
    pcl = labelpath.prototype_contrastive_loss

    def oracle():
        return CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, proto_decay=0.999).step(
            b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))

    def pcl_plus_saw(prototypes, feat, label, *a, **k):
        return pcl(prototypes, feat, label, *a, **k) + wt * saw_differentiable(feat, prototypes, sel, 0.0)
    ref0 = oracle()
    monkeypatch.setattr(labelpath, 'prototype_contrastive_loss', pcl_plus_saw)
    ref = oracle()
    monkeypatch.undo()
    ref_delta = {k: ref['grads'][k] - ref0['grads'][k] for k in ref['grads']}
    ref_delta_norm = torch.sqrt(sum((v.double() ** 2).sum() for v in ref_delta.values())).item()
    delta_tol = 0.06 * (ref0['grad_norm'] + ref['grad_norm']) / ref_delta_norm
    print('oracle: grad norm', ref['grad_norm'], 'without the term', ref0['grad_norm'], 'the term alone', ref_delta_norm,
          'tolerance of its norm', delta_tol)
    assert ref['grad_norm'] >= 1.5 * ref0['grad_norm']
    assert delta_tol == pytest.approx(0.115, abs=0.002)
    gb = {k: v.cuda() for k, v in b.items()}
    keys = ('encoder.resnet.layer4.1.conv3.weight', 'encoder.resnet.layer1.0.conv1.weight', 'encoder.resnet.conv1.weight')

    def make(**kw):
        m = _model(rt, sd)
        m.set_drop_masks(ones, ones)
        return AlignStep(m, protos, **kw)

    def weights_after(classifier=None, **kw):
        """-> step, its outputs, the weights after it, the flat gradient (before clipping), its views of `keys`"""
        st = make(**kw)
        if classifier is not None:
            st.saw['classifier'] = classifier
        out = st.step(gb['images_s'], gb['label_s'], gb['images_t'], gb['regs_t'], 1e-3)
        torch.cuda.synchronize()
        views = {k: st.model._gviews[k].detach().float().cpu().clone() for k in keys}
        return st, out, st.model.flat_p.clone(), st.model.flat_g.clone(), views
    st, (ls, la, gn), w_on, g_on, v_on = weights_after(saw_weight=wt)
    assert st.saw == dict(relax_denom=0.0, selected_classes=None, classifier=None)
    fs, ft = ref['feats']
    P = st.prototypes.cpu()
    want = wt * 0.5 * (saw_restated(fs, P, sel, 0.0)['loss'] + saw_restated(ft, P, sel, 0.0)['loss']).item()
    print('align step: loss_saw', st.loss_saw.item(), want, 'grad norm', gn.sqrt().item(), ref['grad_norm'],
          'loss_align', la.item(), ref['loss_align'])
    assert want > 0.0 and st.loss_saw.item() == pytest.approx(want, rel=0.05)
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)
    assert g_on.double().norm().item() == pytest.approx(gn.sqrt().item(), rel=1e-5)      # flat_g is the unclipped gradient
    _, _, w_on2, g_on2, _ = weights_after(saw_weight=wt)
    assert torch.equal(w_on, w_on2) and torch.equal(g_on, g_on2)
    st0, _, w_zero, _, _ = weights_after(saw_weight=0.0)
    _, (_, _, gn_def), w_def, g_def, v_def = weights_after()
    assert torch.equal(w_zero, w_def) and not torch.equal(w_on, w_def)
    assert st0.loss_saw.item() == 0.0
    assert gn_def.sqrt().item() == pytest.approx(ref0['grad_norm'], rel=0.06)
    # the term's own gradient
    delta_norm = (g_on.double() - g_def.double()).norm().item()
    print('grad norm without the term', gn_def.sqrt().item(), ref0['grad_norm'], 'the term alone', delta_norm, ref_delta_norm)
    assert delta_norm == pytest.approx(ref_delta_norm, rel=delta_tol)
    for k in keys:
        c = _cos(v_on[k] - v_def[k], ref_delta[k])
        print(k, 'cosine of the term\'s gradient', c)
        assert c > 0.9, (k, c)
    # a caller's classifier replaces the prototypes
    other = torch.randn(6, 2048, generator=torch.Generator().manual_seed(2)).cuda()
    st_c, _, w_c, _, _ = weights_after(classifier=other, saw_weight=wt)
    assert not torch.equal(w_c, w_on) and st_c.loss_saw.item() != st.loss_saw.item()
    want_c = wt * 0.5 * (saw_restated(fs, other.cpu(), sel, 0.0)['loss'] + saw_restated(ft, other.cpu(), sel, 0.0)['loss']).item()
    assert st_c.loss_saw.item() == pytest.approx(want_c, rel=0.05)
    with pytest.raises(ValueError):
        make(saw_weight=-1.0)
