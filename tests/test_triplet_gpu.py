"""GPU: the batch-hard triplet loss (rgda_triplet_loss) -- op level against a CPU emulation of the stated contract,
against float64 and against the reference goldens; TripletLoss through autograd; AlignStep(triplet_weight=) against
the CPU stage-2 step composed with the restated term (tests/triplet_ref.py).

Bounds.  Loose (kernel against float64 on the unrounded rows): tests/golden/triplet_tolerances.json, per case 3 x the
deviation of the emulated contract from float64 that tests/golden/derive_triplet_tolerances.py observes on that case's
inputs, and its one mining bound: the true distance of every selected positive / negative lies that close (relative) to
the true extremum.  Against the reference's golden values the reference's own fp32 noise comes on top (triangle
inequality), taken as tests/test_triplet_cpu.py derives it.

Tight (kernel against triplet_emulated: the same roundings; the order of the fp32 sums differs).
Selection.  The emulation sums s_i and G_ij in float64 and rounds once; the kernel sums k products in fp32 in the MFMA's
order.  Every partial sum is at most sum_c |Xh_ic Xh_jc| <= sqrt(s_i s_j) <= (s_i + s_j) / 2 and each of the k additions
rounds by at most 2^-24 of it; with independent signs the k roundings add up to sqrt(k) 2^-24 (s_i + s_j) / 2 for G, so
sqrt(k) 2^-24 (s_i + s_j) for 2 G, the same again for s_i + s_j (two k-long sums), and 3 roundings of the final adds,
3 2^-24 (s_i + s_j): E_ij = (2 sqrt(k) + 3) 2^-24 (s_i + s_j) as one standard deviation.  Two candidates can swap when
their emulated d2 differ by less than the noise of both; the test excuses a row whose best-to-second gap is below
8 E_i, E_i taken with the largest s_j (4 standard deviations on each side; an exact tie of duplicated rows is exact on
both sides and is not excused), and asserts that the excused rows are at
most 1 % of the rows and that EVERY other row selects the emulation's p and n.
Loss.  With equal selections the two sides differ by the order of the k-long fp32 sums of the two squared distances
(sqrt(k) 2^-24 relative, halved by the square root), the device sqrt (correctly rounded) and the order of the sum over
the rows: each hinge d_ap - d_an + margin carries (sqrt(k) / 2 + 2) 2^-24 (d_ap + d_an), and the loss is their mean,
so the bound is (sqrt(k) / 2 + 2 + sqrt(n) ) 2^-24 A with A = mean(d_ap + d_an over the positive hinges) * share /
L computed by the test from the emulation (A is 2 to 400: the hinge is a small difference of two distances); the
sqrt(n) 2^-24 term is the n-long fp32 sum of the hinges in another order.  An excused row that did swap moves its
hinge by at most its gap in distance, 8 E_i / (2 d): added for the excused rows (a share of at most 1 %).
Gradient, relative norm 2^-10 plus the excused rows.  Both sides store bf16, so with equal selections they differ only
where a last-bit difference of an fp32 value flips a bf16 rounding: the fp32 values differ by a few 2^-24 (the
coefficient c / d from a distance that differs by sqrt(k) 2^-25 relative; the emulation rounds products and sums
separately, the kernel may contract them), delta <= 2^-17 of the element for k <= 2048.  A rounding flips with
probability delta / 2^-8 = 2^-9 and then moves the element by one bf16 ulp, at most 2^-7 of it: relative norm
sqrt(2^-9) 2^-7 = 2^-11.5; the bound 2^-10 leaves a factor of 3.  An excused row that swapped moves three gradient rows
entirely: the test compares the gradient on the rows no excused anchor touches (by either side's selection) and
asserts that those are at least 95 % of the rows."""
import json
import os

import numpy as np
import pytest
import torch

from triplet_ref import (CASES, case_inputs, golden_cases, mining_deviation, triplet_differentiable, triplet_emulated,
                         triplet_on_pairs, triplet_restated, variant_cases)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = json.load(open(os.path.join(HERE, 'golden', 'triplet_tolerances.json')))
_CACHE = {}


def reference(name, x, lab, ig):
    """float64 and emulated results of a case, computed once and shared"""
    if name not in _CACHE:
        _CACHE[name] = (triplet_restated(x, lab, ignore_label=ig), triplet_emulated(x, lab, ignore_label=ig))
    return _CACHE[name]


def run(feat, lab, ig=None, weight=1.0, margin=0.3, dfeat=None, accumulate=False, loss=None):
    """-> (loss float, gradient rows bf16 on the CPU, stats tuple, tables dict of numpy arrays)"""
    from regda_amd import ops
    fg = feat if feat.is_cuda else feat.cuda()
    n = lab.numel()
    k = fg.shape[1]
    g = torch.empty(n, k, dtype=BF, device='cuda') if dfeat is None else dfeat
    out, stats, ws = ops.triplet_loss(fg, lab.cuda(), margin, ig, weight, loss=loss, dfeat=g, accumulate=accumulate,
                                      return_ws=True)
    tab = {key: v.cpu().numpy() for key, v in ops.triplet_tables(ws, n).items()}
    return out.item(), g.cpu(), tuple(stats.cpu().tolist()), tab


def _relnorm(got, ref):
    n = np.linalg.norm(ref)
    d = np.linalg.norm(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(d / n) if n else float(d)


def check(name, x, lab, ig, loss, g, stats, tab, loose=True):
    r, e = reference(name, x, lab, ig)
    n, k = x.shape
    u = 2.0 ** -24
    # (a) selection
    E = (2 * np.sqrt(k) + 3) * u * (e['s'].astype(np.float64) + float(e['s'].max()))
    anchors = (e['p'] >= 0) & (e['n'] >= 0)
    # (an exact tie, gap 0, is not excused: identical rows give identical bits on both sides and the lowest index wins)
    excused = anchors & (((e['gap_p'] > 0) & (e['gap_p'] < 8 * E)) | ((e['gap_n'] > 0) & (e['gap_n'] < 8 * E)))
    diff = (tab['p'] != e['p']) | (tab['n'] != e['n'])
    print(name, 'rows', n, 'excused', int(excused.sum()), 'selections that differ', int(diff.sum()),
          'of them excused', int((diff & excused).sum()))
    assert excused.sum() <= 0.01 * n, (name, int(excused.sum()))
    assert not (diff & ~excused).any(), (name, np.nonzero(diff & ~excused)[0][:10])
    assert stats[0] == e['m'], (name, stats, e['m'])
    # (a) loss
    act = e['hinge'] > 0
    swapped = diff & excused
    slack = float((8 * E[swapped] / (2 * np.maximum(np.minimum(e['d_ap'], e['d_an'])[swapped], 1e-6))).sum()) / max(e['m'], 1)
    if e['loss'] > 0:
        A = float((e['d_ap'] + e['d_an'])[act].sum()) / e['m'] / e['loss']
        bound = (np.sqrt(k) / 2 + 2 + np.sqrt(n)) * u * A + slack / e['loss']
        t_l = abs(loss - e['loss']) / e['loss']
        print(name, 'against the emulated contract: loss', loss, e['loss'], 'rel', t_l, 'bound', bound, 'A', A)
        assert t_l <= bound, (name, t_l, bound)
        assert abs(stats[1] - e['active']) <= int(swapped.sum()) + int(0.002 * n), (name, stats, e['active'])
    else:
        assert loss == 0.0 and stats[1] == 0, (name, loss, stats)
    # (a) gradient, on the rows no excused anchor touches
    touched = np.zeros(n, bool)
    for i in np.nonzero(excused)[0]:
        touched[[i, e['p'][i], e['n'][i], tab['p'][i], tab['n'][i]]] = True
    keep = ~touched
    assert keep.sum() >= 0.95 * n
    ge = e['grad'].double().numpy()
    t_g = _relnorm(g.double().numpy()[keep], ge[keep])
    print(name, 'gradient against the emulated contract, relative norm', t_g)
    assert t_g <= 2.0 ** -10, (name, t_g)
    if ig is not None:
        ignored = (lab == ig).numpy()
        assert ignored.any() and not g.float().numpy()[ignored].any()
        assert (tab['p'][ignored] == -1).all() and (tab['n'][ignored] == -1).all()
    # (b) against float64 on the unrounded rows
    md = mining_deviation(x, tab['p'].astype(np.int64), tab['n'].astype(np.int64), r)
    share = float(((tab['p'] != r['p']) | (tab['n'] != r['n'])).mean())
    l_l = abs(loss - r['loss']) / (abs(r['loss']) if r['loss'] else 1.0)
    l_g = _relnorm(g.double().numpy(), r['grad'])
    print(name, 'against float64: loss', loss, r['loss'], 'rel', l_l, 'bound', TOL['bounds'][name]['loss_rel'] if loose else None,
          'grad rel', l_g, 'bound', TOL['bounds'][name]['grad_rel'] if loose else None, 'mining', md,
          'bound', TOL['mining_bound'], 'indices that differ', share)
    assert md <= TOL['mining_bound'], (name, md)
    if loose:
        assert l_l <= TOL['bounds'][name]['loss_rel'], (name, l_l)
        assert l_g <= TOL['bounds'][name]['grad_rel'], (name, l_g)
    return r, e, keep


@pytest.mark.parametrize('name', ['n96_k32', 'n300_k64', 'n130_k96_far', 'n512_k2048', 'n8192_k64'])
def test_triplet_loss_shapes(name):
    """n96_k32: one ragged tile, the smallest k; n300_k64: three tile rows, the last ragged, diagonal and off-diagonal
    tiles; n130_k96_far: no positive hinge; n512_k2048: the production channel count; n8192_k64: the 64 x 64 tile grid
    and the combination of 64 partials per anchor"""
    x, lab = case_inputs(name)
    loss, g, stats, tab = run(x, lab)
    r, e, _ = check(name, x, lab, None, loss, g, stats, tab)
    if name == 'n8192_k64':       # the committed tolerances of this case are current (the CPU test leaves it to this one)
        obs = TOL['observed'][name]
        assert abs(e['loss'] - r['loss']) / r['loss'] == pytest.approx(obs['loss_rel'], rel=1e-3, abs=1e-9)
        assert _relnorm(e['grad'].double().numpy(), r['grad']) == pytest.approx(obs['grad_rel'], rel=1e-3)
    if name == 'n130_k96_far':
        assert loss == 0.0 and stats == (130, 0) and not g.float().any()


@pytest.mark.parametrize('name', ['n300_k64_ignore', 'n300_k64_dup', 'n300_k64_single'])
def test_triplet_loss_edge_conditions(name):
    """rows with ignore_label in every tile; duplicated rows (tied positives go to the lowest index, a duplicate of
    another class puts d_an at the clamp, where it carries no gradient); a class of one (its positive is itself)"""
    x, lab, ig = variant_cases()[name]
    loss, g, stats, tab = run(x, lab, ig)
    r, e, _ = check(name, x, lab, ig, loss, g, stats, tab)
    if name == 'n300_k64_dup':
        assert (tab['p'][150:160] == tab['p'][0:10]).all()              # identical rows select identically ...
        assert not np.isin(tab['p'], np.arange(150, 160)).any()         # ... and never the later copy of a tie
        assert (tab['n'][20:25] == np.arange(200, 205)).all() and (tab['d_an'][20:25] == 0).all()
        assert (tab['hinge'][20:25] > 0).all()
    if name == 'n300_k64_single':
        assert tab['p'][17] == 17 and tab['d_ap'][17] == 0.0


def test_triplet_loss_matches_the_reference_goldens(gold):
    """(c): the loose bounds plus the reference's own fp32 noise, derived as in tests/test_triplet_cpu.py"""
    for c in golden_cases(gold('triplet.npz')):
        loss, g, stats, tab = run(c['x'], c['labels'], margin=c['margin'])
        if c['loss'] == 0.0:
            assert loss == 0.0 and not g.float().any()
            continue
        r = triplet_restated(c['x'], c['labels'], c['margin'])
        f = triplet_restated(c['x'], c['labels'], c['margin'], dtype=np.float32)
        floor = 2.0 ** -23 * float(r['d_ap'][r['p'] >= 0].mean()) / r['loss']
        noise_l = 3 * max(abs(f['loss'] - r['loss']) / r['loss'], floor)
        noise_g = 3 * max(_relnorm(f['grad'], r['grad']), 2.0 ** -23)
        lrel = abs(loss - c['loss']) / c['loss']
        grel = _relnorm(g.double().numpy(), c['grad'].double().numpy())
        print(c['name'], 'loss', loss, c['loss'], 'rel', lrel, 'grad rel', grel)
        assert lrel <= TOL['bounds'][c['name']]['loss_rel'] + noise_l, (c['name'], lrel)
        assert grel <= TOL['bounds'][c['name']]['grad_rel'] + noise_g, (c['name'], grel)


def test_batch_slice_read_in_place_weight_wide_rows_and_accumulate():
    """feat[1:3] of a (4, 64, 8, 12) map is read through its strides; weight 0.5; gradient rows of 72 columns whose last
    8 stay; accumulate on a pre-filled buffer against accumulate = 0"""
    from regda_amd import ops
    gen = torch.Generator().manual_seed(21)
    lab = torch.randint(0, 3, (2 * 96,), generator=gen)
    lab[5::11] = -1
    cent = torch.randn(3, 64, generator=gen)
    rows = 0.9 * cent[lab.clamp(min=0)] + torch.randn(192, 64, generator=gen)
    full = torch.randn(4, 64, 8, 12, generator=gen)
    full[1:3] = rows.view(2, 8, 12, 64).permute(0, 3, 1, 2)
    fg = full.cuda()
    sl = fg[1:3]
    assert not sl.is_contiguous() or sl.data_ptr() != fg.data_ptr()
    loss1, g1, stats1, tab1 = run(sl, lab, -1)
    r, e1, keep = check('slice', rows, lab, -1, loss1, g1, stats1, tab1, loose=False)
    assert 0 < e1['active'] < e1['m']
    e = triplet_emulated(rows, lab, ignore_label=-1, weight=0.5)
    loss, g, stats, tab = run(sl, lab, -1, weight=0.5)
    assert all(np.array_equal(tab[key], tab1[key]) for key in tab) and stats == stats1      # the weight moves no selection
    assert loss == pytest.approx(0.5 * loss1, rel=1e-6)
    assert _relnorm(g.double().numpy()[keep], e['grad'].double().numpy()[keep]) <= 2.0 ** -10
    # the same rows given as an (n, k) matrix: bit-identical
    loss2, g2, stats2, _ = run(rows, lab, -1, weight=0.5)
    assert loss2 == loss and torch.equal(g2, g) and stats2 == stats
    # accumulate onto a pre-filled wide buffer; the loss tensor accumulates too
    prior = (torch.randn(192, 72, generator=gen) * e['grad'].float().abs().max()).bfloat16()
    buf = prior.cuda()
    acc = torch.full((1,), 2.0, device='cuda')
    ops.triplet_loss(sl, lab.cuda(), 0.3, -1, 0.5, loss=acc, dfeat=buf, accumulate=True)
    assert acc.item() == pytest.approx(2.0 + loss, rel=1e-6)
    want = triplet_emulated(rows, lab, ignore_label=-1, weight=0.5, prior=prior[:, :64])['grad']
    got = buf.cpu()
    assert torch.equal(got[:, 64:], prior[:, 64:])
    untouched = (g.float().abs().sum(1) == 0)
    assert untouched.any() and torch.equal(got[untouched, :64], prior[untouched, :64])
    assert _relnorm(got[:, :64].double().numpy()[keep], want.double().numpy()[keep]) <= 2.0 ** -10     # rounded once, as g
    # accumulate = 0 overwrites a pre-filled buffer, the untouched rows with zeros
    buf = prior.cuda()
    ops.triplet_loss(sl, lab.cuda(), 0.3, -1, 0.5, dfeat=buf, accumulate=False)
    assert torch.equal(buf.cpu()[:, :64], g) and torch.equal(buf.cpu()[:, 64:], prior[:, 64:])


def test_one_class_only_gives_zero_loss_zero_gradient_and_empty_stats():
    x, lab = case_inputs('n300_k64')
    for labels, ig in ((torch.full_like(lab, 3), None), (torch.where(lab == 2, lab, torch.full_like(lab, -1)), -1),
                       (torch.full_like(lab, -1), -1)):
        buf = torch.full((300, 64), 7.0, dtype=BF, device='cuda')
        loss, g, stats, tab = run(x, labels, ig, dfeat=buf)
        assert loss == 0.0 and stats == (0, 0) and not g.float().any()
        assert (tab['n'] == -1).all() and (tab['hinge'] == 0).all()


def test_two_calls_are_bit_identical():
    for name in ('n300_k64', 'n8192_k64'):
        x, lab = case_inputs(name)
        xg = x.cuda()
        a = run(xg, lab)
        b = run(xg, lab)
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and a[2] == b[2]
        for key in a[3]:
            assert np.array_equal(a[3][key], b[3][key]), key


def test_module_through_autograd_equals_the_op():
    """(d): TripletLoss on a (2, 64, 8, 8) map, differentiable; equal to the op on the same map and, for rows, to the
    NCHW form"""
    from regda_amd.gast import TripletLoss
    gen = torch.Generator().manual_seed(31)
    lab = torch.randint(0, 3, (128,), generator=gen)
    lab[::9] = -1
    cent = torch.randn(3, 64, generator=gen)
    rows = 1.0 * cent[lab.clamp(min=0)] + torch.randn(128, 64, generator=gen)
    fmap = rows.view(2, 8, 8, 64).permute(0, 3, 1, 2).contiguous()
    loss_op, g_op, stats, _ = run(fmap, lab, -1)
    assert 0 < stats[1] <= stats[0]
    f = fmap.cuda().requires_grad_(True)
    out = TripletLoss(ignore_label=-1)(f, lab.cuda())
    (3.0 * out).backward()
    assert out.item() == loss_op
    want = 3.0 * g_op.float().view(2, 8, 8, 64).permute(0, 3, 1, 2)
    assert torch.equal(f.grad.cpu(), want)
    x = rows.cuda().requires_grad_(True)
    out2 = TripletLoss(ignore_label=-1)(x, lab.cuda())
    out2.backward()
    assert out2.item() == loss_op and torch.equal(x.grad.cpu(), g_op.float())
    # and the value: float64 autograd of the definition
    xd = rows.double().requires_grad_(True)
    ref = triplet_differentiable(xd, lab, 0.3, -1)
    ref.backward()
    assert out2.item() == pytest.approx(ref.item(), rel=1e-4)
    assert _relnorm(x.grad.cpu().double().numpy(), xd.grad.numpy()) <= 0.1


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return (a @ b / (a.norm() * b.norm())).item()


WT = 1.0          # the term's weight in the step test (see its docstring)


def test_align_step_triplet_weight_matches_the_composed_oracle(monkeypatch):
    """AlignStep(triplet_weight=w) against the composed oracle: the CPU stage-2 step (oracle.step.CpuAlignStep) plus the
    restated term on the oracle's own features with the STEP's downscaled labels (step.last_label_s_down and
    step.last_label_t, ignore label -1), composed by wrapping the oracle's two PCL calls as
    tests/test_pixel_contrast_gpu.py does: each adds w * T(feat rows), and the step halves their sum.

    Shape: the smallest the align tests use (2 + 2 tiles of 128^2, 8 x 8 feature pixels per image: 128 rows per domain,
    2048 channels).  Batch-hard mining is discontinuous: the bf16 network's features move some anchors to another
    hardest pair than the oracle's fp32 features select, and each such anchor redirects three gradient rows.  So, as the
    contrast test evaluates the oracle's term on the rows the step selected, the oracle's term here is evaluated on the
    PAIRS the step selected (step.last_triplet: triplet_ref.triplet_on_pairs); that the step selected them from the
    right inputs is checked separately: on the oracle's features the distance of every pair the step selected lies
    within 5 % of the true extremum of the step's labels (the features of the two networks differ by about 1 %; a pair
    mined on the other domain's features or with the other domain's labels is off by tens of percent), and loss_triplet
    is compared with the full restatement (mining included) on the oracle's features, rel 0.05 as for loss_contrast
    and loss_white.

    The instance-normalised features have distances of 30 to 60 and an untrained network separates no class, so every
    hinge is positive and the term is about 18; with w = 1 it doubles the step's gradient: the oracle's norms with and
    without it are asserted to differ by >= 1.5, so a missing, halved or doubled gradient moves the norm outside the
    0.06 of the stage-2 step tests.  The term's own gradient (the flat gradient with the term minus the one without,
    before clipping) is compared with the oracle's difference: cosines > 0.9 and norm within 0.12, the bounds and
    reasoning of test_align_step_whiten_weight.  The updated weights: the classifier's update within 0.08 and the
    update directions' cosines, as tests/test_align_gpu.py asserts them.  triplet_weight = 0 is bit-identical to a step
    built without the argument."""
    from oracle import labelpath, model as omodel
    from oracle.step import CpuAlignStep
    from regda_amd.align import AlignStep
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.synthetic import make_batch
    rt, wt = 'resnet17t', WT
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
        out = st.step(gb['images_s'], gb['label_s'], gb['images_t'], gb['regs_t'], 1e-3)
        torch.cuda.synchronize()
        views = {k: m._gviews[k].detach().float().cpu().clone() for k in keys}
        return st, out, m.flat_g.clone(), views, {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    st, (_, _, gn), g_on, v_on, w_on = run_step(triplet_weight=wt)
    _, (_, _, gn_def), g_def, v_def, w_def = run_step()
    _, _, g_zero, _, w_zero = run_step(triplet_weight=0.0)
    assert torch.equal(g_zero, g_def)
    for k in w_def:
        assert torch.equal(w_zero[k], w_def[k]), k
    assert st.triplet == dict(margin=0.3)
    labs = [st.last_label_s_down.cpu().reshape(-1), st.last_label_t.cpu().reshape(-1)]
    stats = [tuple(t['stats'].cpu().tolist()) for t in st.last_triplet]
    pairs = [(t['p'].cpu().long(), t['n'].cpu().long()) for t in st.last_triplet]
    print('step: (m, positive hinges) per domain', stats)
    for lab, (m_rows, act) in zip(labs, stats):
        assert m_rows == int((lab != -1).sum()) and m_rows >= 32 and act >= 1

    def rows_of(feat):
        return feat.permute(0, 2, 3, 1).reshape(-1, feat.shape[1])
    pcl, calls, feats = labelpath.prototype_contrastive_loss, [], []

    def pcl_plus_triplet(prototypes, feat, label, *a, **k):
        sp, sq = pairs[len(calls)]
        calls.append(label)
        feats.append(feat.detach())
        return pcl(prototypes, feat, label, *a, **k) + wt * triplet_on_pairs(rows_of(feat), sp, sq, 0.3)

    def oracle():
        return CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, proto_decay=0.999).step(
            b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))
    ref0 = oracle()
    monkeypatch.setattr(labelpath, 'prototype_contrastive_loss', pcl_plus_triplet)
    cpu = CpuAlignStep(sd, protos, resnet_type=rt, lr=1e-3, proto_decay=0.999)
    ref = cpu.step(b['images_s'], b['label_s'], b['images_t'], b['regs_t'], (ones, ones), (ones, ones))
    monkeypatch.undo()
    assert len(calls) == 2
    print('oracle: grad norm', ref['grad_norm'], 'without the term', ref0['grad_norm'])
    assert ref['grad_norm'] >= 1.5 * ref0['grad_norm']
    for side in range(2):
        moved = (calls[side].reshape(-1) != labs[side]).float().mean().item()
        print('side', side, 'share of downscaled labels that differ from the oracle\'s', moved)
        assert moved <= 0.05

    parts = [triplet_restated(rows_of(f), lab, 0.3, -1) for f, lab in zip(feats, labs)]
    for side, (f, part) in enumerate(zip(feats, parts)):           # the step mined the right rows with the right labels
        md = mining_deviation(rows_of(f), pairs[side][0].numpy(), pairs[side][1].numpy(), part)
        share = float(((pairs[side][0].numpy() != part['p']) | (pairs[side][1].numpy() != part['n'])).mean())
        print('side', side, 'selected distances against the oracle\'s extremum', md, 'share of rows with another pair', share)
        assert part['m'] == stats[side][0] and md <= 0.05, (side, md)
    want = wt * 0.5 * sum(p['loss'] for p in parts)
    print('loss_triplet', st.loss_triplet.item(), want, 'grad norm', gn.sqrt().item(), ref['grad_norm'],
          'oracle (m, positive hinges)', [(p['m'], p['active']) for p in parts])
    assert want > 0.0 and st.loss_triplet.item() == pytest.approx(want, rel=0.05)
    assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)
    assert gn_def.sqrt().item() == pytest.approx(ref0['grad_norm'], rel=0.06)

    ref_delta = {k: ref['grads'][k] - ref0['grads'][k] for k in ref['grads']}
    ref_delta_norm = torch.sqrt(sum((v.double() ** 2).sum() for v in ref_delta.values())).item()
    delta_norm = (g_on.double() - g_def.double()).norm().item()
    print('the term alone', delta_norm, ref_delta_norm)
    assert delta_norm == pytest.approx(ref_delta_norm, rel=0.12)
    for k in keys:
        c = _cos(v_on[k] - v_def[k], ref_delta[k])
        print(k, 'cosine of the term\'s gradient', c)
        assert c > 0.9, (k, c)

    for k, tol in (('encoder.resnet.layer4.1.conv3.weight', 0.97), ('encoder.resnet.conv1.weight', 0.9)):
        c = _cos(cpu.sd[k].detach() - sd[k], w_on[k] - sd[k])
        print(k, 'cosine of the update', c)
        assert c > tol, (k, c)
    k = 'layer5.conv_last.4.weight'
    d_ref, d_got = cpu.sd[k].detach() - sd[k], w_on[k] - sd[k]
    assert ((d_got - d_ref).norm() / d_ref.norm()).item() < 0.08
