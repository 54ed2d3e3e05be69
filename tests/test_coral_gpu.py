"""GPU: CORAL (rgda_coral_loss) -- op level against the reference goldens and, at the production shape, against a CPU
emulation of the stated contract; the drop-in Aligner (align_domain through Deeplabv2's autograd path, update_avg /
init_avg); the stage-1 SourceStep and AlignStep(align_domain=True) against CPU steps composed from the oracle."""
import numpy as np
import pytest
import torch

from test_coral_cpu import _rows, coral_cases, coral_restated

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def run(xs, xt, weight=1.0):
    from regda_amd import ops
    gs = torch.empty(_rows(xs).shape, dtype=BF, device='cuda')
    gt = torch.empty(_rows(xt).shape, dtype=BF, device='cuda')
    loss = ops.coral_loss(xs.cuda(), xt.cuda(), weight, dfeat_s=gs, dfeat_t=gt)
    return loss, gs, gt


def test_coral_loss_matches_the_reference_goldens(gold):
    g = gold('coral.npz')
    for i, xs, xt in coral_cases(g):
        loss, gs, gt = run(xs, xt)
        # bf16 centred operands (relative 2^-9 per element) in products of >= 32 rows; the gradient is stored in bf16
        assert loss.item() == pytest.approx(float(g[f'loss{i}']), rel=1e-2), i
        for got, ref in ((gs, g[f'gs{i}']), (gt, g[f'gt{i}'])):
            ref = _rows(torch.from_numpy(ref))
            err = (got.float().cpu() - ref).norm() / ref.norm()
            assert err.item() < 1.5e-2, (i, err.item())


def emulate_contract(xs, xt):
    """The arithmetic contract of rgda_coral_loss on the CPU: fp32 means, centred rows rounded to bf16 once, fp32 sums,
    bf16(D) in the gradient product."""
    d, ns, nt = xs.shape[1], xs.shape[0], xt.shape[0]
    cs = (xs - xs.mean(0)).to(BF).float()
    ct = (xt - xt.mean(0)).to(BF).float()
    D = cs.T @ cs / (ns - 1) - ct.T @ ct / (nt - 1)
    Db = D.to(BF).float()
    return (D * D).sum() / (4 * d * d), cs @ Db / (d * d * (ns - 1)), -(ct @ Db) / (d * d * (nt - 1))


def test_coral_loss_production_shape_against_the_contract_and_fp32():
    """2 x 8192 x 2048 (8 + 8 images of 512^2 at output stride 16).
    Tight bounds, against the emulated contract (same roundings, only the fp32 summation order differs): loss rel 1e-4;
    gradient relative norm 5e-3 (its bf16 store, 2^-9 relative per element = 1.1e-3 RMS, plus the few elements of bf16(D)
    that round the other way from a last-bit difference of D).
    Loose bounds, against fp64 on the unrounded features: every centred element carries a relative rounding error of at
    most 2^-9 (RMS 2^-9 / sqrt(3) = 1.1e-3), independent across elements, so an element of C = Xc^T Xc / (n - 1) moves by
    about sqrt(2) * 1.1e-3 of its own scale; with source and target covariances that differ in scale, |D| ~ |C| and the
    loss (a sum of 4M such squares) moves far less than that -- bound 5e-3.  The gradient carries three independent
    bf16 roundings (X, D, the stored result): RMS sqrt(3) * 1.1e-3 = 2e-3 relative -- bound 1e-2."""
    gen = torch.Generator().manual_seed(8192)
    b, d, h, w = 8, 2048, 32, 32
    fs = torch.randn(b, d, h, w, generator=gen)
    ft = torch.randn(b, d, h, w, generator=gen) * 1.2 + 0.1
    loss, gs, gt = run(fs, ft)
    xs, xt = _rows(fs), _rows(ft)
    el, egs, egt = emulate_contract(xs, xt)
    assert abs(loss.item() - el.item()) <= 1e-4 * el.item()
    for got, ref in ((gs, egs), (gt, egt)):
        assert ((got.float().cpu() - ref).norm() / ref.norm()).item() < 5e-3
    rl, rgs, rgt = coral_restated(xs, xt)
    assert abs(loss.item() - rl.item()) <= 5e-3 * rl.item()
    for got, ref in ((gs, rgs), (gt, rgt)):
        assert ((got.double().cpu() - ref).norm() / ref.norm()).item() < 1e-2
    # two identical calls are bit-identical (no atomics; split-K partials reduced in a fixed order)
    loss2, gs2, gt2 = run(fs, ft)
    assert torch.equal(loss, loss2) and torch.equal(gs, gs2) and torch.equal(gt, gt2)


def test_coral_loss_accumulate_weight_and_identical_domains():
    from regda_amd import ops
    gen = torch.Generator().manual_seed(5)
    fs = torch.randn(3, 256, 8, 12, generator=gen)
    ft = torch.randn(2, 256, 16, 8, generator=gen) * 0.7          # ns = 288 != nt = 256
    loss, gs, gt = run(fs, ft)
    rl, rgs, rgt = coral_restated(_rows(fs), _rows(ft))
    assert loss.item() == pytest.approx(rl.item(), rel=5e-3)
    base_s = torch.randn(gs.shape, generator=gen).mul(rgs.abs().max().item()).to(BF).cuda()
    base_t = torch.randn(gt.shape, generator=gen).mul(rgt.abs().max().item()).to(BF).cuda()
    acc_s, acc_t = base_s.clone(), base_t.clone()
    lacc = torch.full((1,), 2.0, device='cuda')
    ops.coral_loss(fs.cuda(), ft.cuda(), 0.5, loss=lacc, dfeat_s=acc_s, dfeat_t=acc_t, accumulate=True)
    assert lacc.item() == pytest.approx(2.0 + 0.5 * loss.item(), rel=1e-6)
    for acc, base, ref in ((acc_s, base_s, rgs), (acc_t, base_t, rgt)):
        want = base.double().cpu() + 0.5 * ref
        # fp32 add, one bf16 rounding of the sum: |err| <= 2^-8 |sum| per element, plus the gradient's own error
        err = (acc.double().cpu() - want).abs()
        assert (err <= 2 ** -8 * want.abs() + 1e-2 * ref.abs().max().item()).all()
    # the same features on both sides: loss and gradient at rounding level (D within a few fp32 ulps of C of 0)
    loss0, g0s, g0t = run(fs, fs.clone())
    assert 0.0 <= loss0.item() <= 1e-12 * rl.item()
    for g0, ref in ((g0s, rgs), (g0t, rgt)):
        assert g0.float().abs().max().item() <= 1e-5 * ref.abs().max().item()
    # d = 96 (one and a half 64-channel staging tiles, less than one 128 x 128 product tile), both domains batch and
    # channel slices of wider maps, read in place through their strides (image stride > channels x channel stride), dfeat
    # wider than d: against the emulated contract, with the bounds of the production-shape test (like roundings on both
    # sides, so they do not depend on the shape)
    s96 = (torch.randn(4, 128, 8, 12, generator=gen).cuda()[1:, 16:112],
           torch.randn(3, 128, 16, 8, generator=gen).mul(0.7).cuda()[:2, 16:112])
    assert not s96[0].is_contiguous() and tuple(s96[0].shape) == (3, 96, 8, 12) and tuple(s96[1].shape) == (2, 96, 16, 8)
    wide = [torch.zeros(n, 104, dtype=BF, device='cuda') for n in (288, 256)]
    l96 = ops.coral_loss(*s96, dfeat_s=wide[0][:, :96], dfeat_t=wide[1][:, :96])
    el, *eg = emulate_contract(_rows(s96[0].cpu()), _rows(s96[1].cpu()))
    print('coral d=96: loss', l96.item(), 'contract', el.item())
    assert abs(l96.item() - el.item()) <= 1e-4 * el.item()
    for got, ref in zip(wide, eg):
        err = ((got[:, :96].float().cpu() - ref).norm() / ref.norm()).item()
        print('coral d=96: gradient relative norm', err)
        assert err < 5e-3 and float(got[:, 96:].float().abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.coral_loss(fs[:, :100].cuda(), ft[:, :100].cuda())
    with pytest.raises(ValueError):
        ops.coral_loss(fs[:1, :, :1, :1].cuda(), ft.cuda())


def _model(rt, sd):
    from regda_amd.models.Encoder import Deeplabv2
    m = Deeplabv2(dict(backbone=dict(resnet_type=rt, output_stride=16, pretrained=False), multi_layer=True, cascade=False,
                       use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048, num_classes=6,
                       is_ins_norm=True))
    m.load_state_dict(sd, strict=True)
    return m


def cpu_stage1(sd, rt, xs, lab, xt, masks_s=None, masks_t=None, with_ce=True):
    """tools/train_src.py:117-140 with --align-domain 1 composed on the CPU oracle: two train-mode forwards,
    loss_calc + CORAL (restated above), autograd gradients."""
    from oracle import labelpath, model as omodel
    sd = {k: v.clone() for k, v in sd.items()}
    names = omodel.param_names(sd)
    for k in names:
        sd[k].requires_grad_(True)
    s1, s2, fs = omodel.forward(sd, xs, True, masks_s, rt, {})
    _, _, ft = omodel.forward(sd, xt, True, masks_t, rt, {})
    loss_seg = labelpath.loss_calc([s1, s2], lab, -1)
    loss_dom = coral_restated(_rows(fs), _rows(ft))[0].float()
    loss = loss_dom + (loss_seg if with_ce else 0)
    grads = torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(sd[k]) if g is None else g) for k, g in zip(names, grads)}
    gn = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).item()
    return dict(loss_seg=float(loss_seg.detach()), loss_domain=float(loss_dom.detach()), grad_norm=gn, grads=grads,
                feats=(fs.detach(), ft.detach()))


def _cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return (a @ b / (a.norm() * b.norm())).item()


def test_aligner_align_domain_through_the_model_autograd_path():
    """The drop-in surface as tools/train_src.py uses it: model(xs), model(xt), aligner.align_domain(feat_s, feat_t),
    loss.backward().  CORAL alone (no CE), so the parameter gradients are the CORAL gradient only."""
    from oracle import model as omodel
    from regda_amd.gast.alignment import Aligner
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, 6, seed=21)
    gen = torch.Generator().manual_seed(3)
    xs, xt = torch.randn(2, 3, 128, 128, generator=gen), torch.randn(2, 3, 128, 128, generator=gen) * 1.3
    ref = cpu_stage1(sd, rt, xs, torch.zeros(2, 128, 128, dtype=torch.long), xt, with_ce=False)
    m = _model(rt, sd)
    m.train()
    al = Aligner(None, feat_channels=2048, class_num=6)
    _, _, fs = m(xs.cuda())
    _, _, ft = m(xt.cuda())
    loss = al.align_domain(fs, ft)
    loss.backward()
    assert loss.item() == pytest.approx(ref['loss_domain'], rel=0.05)
    named = dict(m.named_parameters())
    for k in ('encoder.resnet.layer4.1.conv3.weight', 'encoder.resnet.layer1.0.conv1.weight', 'encoder.resnet.conv1.weight'):
        c = _cos(named[k].grad.cpu(), ref['grads'][k])
        assert c > 0.9, (k, c)
    # the classifier heads do not see CORAL
    assert named['layer5.conv_last.4.weight'].grad.abs().max().item() == 0.0
    with pytest.raises(AssertionError):
        al.align_domain(fs, ft[:1])


def test_aligner_update_avg_init_avg_match_the_reference(gold):
    from regda_amd.gast.alignment import Aligner
    g = gold('proto_init.npz')
    al = Aligner(None, feat_channels=64, class_num=6, ignore_label=-1)
    for i in range(3):
        al.update_avg(torch.from_numpy(g[f'feat{i}']).cuda(), torch.from_numpy(g[f'lab{i}'].astype(np.int64)).cuda())
    al.init_avg()
    assert np.array_equal(al.data_cnt.cpu().numpy(), g['data_cnt'])           # counts exact
    np.testing.assert_allclose(al.data_sum.cpu().numpy(), g['data_sum'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(al.prototypes.cpu().numpy(), g['protos'], rtol=1e-5, atol=1e-6)
    assert float(g['data_cnt'][5, 0]) == 0 and al.prototypes[5].abs().max().item() == 0.0


def test_source_step_matches_the_reference_golden(gold):
    """SourceStep(align_domain=True) on the ResNet-101 stage-1 golden (tools/train_src.py:117-140, --align-domain 1)."""
    from oracle import model as omodel
    from regda_amd.source import SourceStep
    g, a = gold('model_small.npz'), gold('src_small.npz')
    sd = omodel.init_state_dict('resnet101', 6, seed=1)
    m = _model('resnet101', sd)
    m.set_drop_masks(torch.from_numpy(np.concatenate([a['m5'][0], a['m5'][1]])),
                     torch.from_numpy(np.concatenate([a['m6'][0], a['m6'][1]])))
    st = SourceStep(m, align_domain=True)
    t = lambda k: torch.from_numpy(g[k]).cuda()        # noqa: E731
    ls, ld, gn = st.step(t('xs'), t('lab_s').long(), t('xt'), lr=0.0)
    # stated tolerances: bf16 network; CORAL is a difference of two covariances of bf16 features
    assert ls.item() == pytest.approx(float(a['loss_seg']), rel=0.02)
    assert ld.item() == pytest.approx(float(a['loss_domain']), rel=0.05)
    assert gn.sqrt().item() == pytest.approx(float(a['grad_norm']), rel=0.06)


def _batch(seed, b=2, size=128, ignore_all=False):
    from regda_amd.synthetic import make_batch
    bb = make_batch(b=b, size=size, seed=seed, device='cpu')
    lab = bb['label_s'].clone()
    if ignore_all:
        lab.fill_(-1)
    return bb['images_s'], lab, bb['images_t']


@pytest.mark.parametrize('ignore_all', [False, True])
def test_source_step_matches_the_composed_oracle(ignore_all):
    """resnet17t: losses and gradient norm against the CPU stage-1 step; with every source label ignored the CE and its
    gradient are 0 (the reference's mean over all pixels) and the whole gradient is CORAL's: per-tensor cosines of the
    flat gradient (gradients, not weight deltas: weight decay dwarfs a CORAL-only gradient)."""
    from oracle import model as omodel
    from regda_amd.source import SourceStep
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, 6, seed=6)
    xs, lab, xt = _batch(11, ignore_all=ignore_all)
    ones = torch.ones(2, 512)
    ref = cpu_stage1(sd, rt, xs, lab, xt, (ones, ones), (ones, ones))
    m = _model(rt, sd)
    m.set_drop_masks(ones, ones)
    st = SourceStep(m, align_domain=True)
    ls, ld, gn = st.step(xs.cuda(), lab.cuda(), xt.cuda(), lr=1e-3)
    assert ld.item() == pytest.approx(ref['loss_domain'], rel=0.05)
    if ignore_all:
        assert ls.item() == 0.0
        views = m._gviews           # per-parameter views of model.flat_g, the step's gradient
        for k in ('encoder.resnet.layer4.1.conv3.weight', 'encoder.resnet.layer2.0.conv2.weight',
                  'encoder.resnet.conv1.weight'):
            c = _cos(views[k].cpu(), ref['grads'][k])
            assert c > 0.9, (k, c)
        assert views['layer5.conv_last.4.weight'].abs().max().item() == 0.0
        assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.1)
    else:
        assert ls.item() == pytest.approx(ref['loss_seg'], rel=0.02)
        assert gn.sqrt().item() == pytest.approx(ref['grad_norm'], rel=0.06)


def _weights_after(make_step, run):
    out = []
    for _ in range(2):
        st = make_step()
        run(st)
        torch.cuda.synchronize()
        out.append(st.model.flat_p.clone())
    return out


def test_source_step_without_alignment_and_determinism():
    from oracle import model as omodel
    from regda_amd.source import SourceStep
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, 6, seed=8)
    xs, lab, xt = _batch(12)
    ones = torch.ones(2, 512)

    def make(align):
        def mk():
            m = _model(rt, sd)
            m.set_drop_masks(ones, ones)
            return SourceStep(m, align_domain=align)
        return mk
    for align in (True, False):
        w1, w2 = _weights_after(make(align), lambda st: st.step(xs.cuda(), lab.cuda(), xt.cuda() if align else None, 1e-3))
        assert torch.equal(w1, w2), align
    # align_domain off: no target forward, loss_domain 0, CE as the oracle's
    st = make(False)()
    ls, ld, _ = st.step(xs.cuda(), lab.cuda(), None, 1e-3)
    from oracle import labelpath
    with torch.no_grad():
        s1, s2, _ = omodel.forward(sd, xs, True, (ones, ones), rt)
        ref = labelpath.loss_calc([s1, s2], lab, -1).item()
    assert ld.item() == 0.0 and ls.item() == pytest.approx(ref, rel=0.02)
    with pytest.raises(ValueError):
        make(True)().step(xs.cuda(), lab.cuda(), None, 1e-3)
    with pytest.raises(NotImplementedError):
        st.record_plan()


def test_align_step_align_domain():
    """AlignStep(align_domain=True): loss_domain against CORAL of the oracle's forward features; the default step is
    unchanged (bit-identical weights with align_domain=False given explicitly); two runs bit-identical."""
    from oracle import model as omodel
    from regda_amd.align import AlignStep
    from regda_amd.synthetic import make_batch
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, 6, seed=6)
    b = make_batch(b=2, size=128, seed=11, device='cpu')
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(1))
    ones = torch.ones(2, 512)
    with torch.no_grad():
        _, _, fs = omodel.forward(sd, b['images_s'], True, (ones, ones), rt)
        _, _, ft = omodel.forward(sd, b['images_t'], True, (ones, ones), rt)
        ref = coral_restated(_rows(fs), _rows(ft))[0].item()
    gb = {k: v.cuda() for k, v in b.items()}

    def make(**kw):
        def mk():
            m = _model(rt, sd)
            m.set_drop_masks(ones, ones)
            return AlignStep(m, protos, **kw)
        return mk
    last = {}

    def run(st):
        last['out'] = st.step(gb['images_s'], gb['label_s'], gb['images_t'], gb['regs_t'], 1e-3)
        last['st'] = st
    w_on = _weights_after(make(align_domain=True), run)
    assert torch.equal(w_on[0], w_on[1])
    assert last['st'].loss_domain.item() == pytest.approx(ref, rel=0.05)
    w_def = _weights_after(make(), run)
    w_off = _weights_after(make(align_domain=False), run)
    assert torch.equal(w_def[0], w_off[0]) and torch.equal(w_def[0], w_def[1])
    assert not torch.equal(w_def[0], w_on[0])
