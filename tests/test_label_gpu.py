"""GPU parity of the label path (pseudo_selection, LRH, label_refine, update_prototype, loss, teacher)
through the C ABI, against the golden vectors of the reference and against the oracle on seeded
inputs.  Integer results must be bit-identical; float tolerances are stated per test.
Per element at edge shapes and on every route: tests/label_cases.py, test_label_cases_cpu.py, test_label_passes_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import labels as olab
from oracle import labelpath as opath

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
    from regda_amd.utils.local_region_homog import Homogenizer
    from regda_amd.gast.pseudo_generation import pseudo_selection
    from regda_amd.gast.alignment import Aligner, DownscaleLabel
    from regda_amd.gast.balance import CrossEntropy, ClassBalance
    from regda_amd.utils.tools import loss_calc
    from regda_amd import ops
    import types
    return types.SimpleNamespace(**locals())


def cu(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dt is not None:
        t = t.to(dt)
    return t.cuda()


def test_lrh_golden_bit_exact(mods, gold):
    g = gold('lrh.npz')
    for i in range(int(g['n'])):
        h = mods.Homogenizer(percent=float(g[f'pct{i}']), class_num=6, ignore_label=-1)
        out = h(cu(g[f'lab{i}'], torch.int64), cu(g[f'reg{i}'], torch.int64)).cpu().numpy()
        assert np.array_equal(out, g[f'out{i}'].astype(np.int64)), f'golden case {i}'


@pytest.mark.parametrize('shape,nreg', [((8, 512, 512), 250), ((2, 512, 512), 3000), ((1, 7, 5), 3), ((3, 100, 37), 60)])
def test_lrh_vs_oracle_seeded(mods, shape, nreg):
    rng = np.random.default_rng(123)
    b, h, w = shape
    regs = np.zeros(shape, np.int64)
    for i in range(b):
        for r in range(1, nreg + 1):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            regs[i, y0:y0 + rng.integers(1, max(2, h // 4)), x0:x0 + rng.integers(1, max(2, w // 4))] = r
    lab = rng.integers(-1, 6, size=shape).astype(np.int64)
    blk = np.kron(rng.integers(-1, 6, size=(b, (h + 31) // 32, (w + 31) // 32)), np.ones((32, 32), np.int64))[:, :h, :w]
    lab = np.where(rng.random(shape) < 0.85, blk, lab)
    h_ = mods.Homogenizer(percent=0.5, class_num=6, ignore_label=-1)
    out = h_(cu(lab), cu(regs)).cpu().numpy()
    assert np.array_equal(out, olab.homogenize(lab, regs, 0.5, 6, -1))
    # properties at full size: idempotent on homogenised regions, region 0 untouched
    assert np.array_equal(out[regs == 0], lab[regs == 0])
    out2 = h_(cu(out), cu(regs)).cpu().numpy()
    changed = out != lab
    assert np.array_equal(out2[changed], out[changed])


def test_lrh_errors_and_empty(mods):
    h = mods.Homogenizer(percent=0.5, class_num=6, ignore_label=-1, max_regions=8)
    lab = torch.zeros((1, 4, 4), dtype=torch.int64, device='cuda')
    reg = torch.full((1, 4, 4), 9, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError):
        h(lab, reg)
    with pytest.raises(AssertionError):
        h(lab[0], reg[0])
    with pytest.raises(RuntimeError):
        h(lab.cpu(), reg.cpu())
    e = h(torch.zeros((2, 0, 4), dtype=torch.int64, device='cuda'), torch.zeros((2, 0, 4), dtype=torch.int64, device='cuda'))
    assert e.shape == (2, 0, 4)


def test_pseudo_selection_golden_bit_exact(mods, gold):
    g = gold('pseudo.npz')
    for i in range(int(g['n'])):
        out = mods.pseudo_selection(cu(g[f'in{i}']), 0.8, 0.6, 'tensor', -1).cpu().numpy()
        assert np.array_equal(out, g[f'out{i}'].astype(np.int64)), f'golden case {i}'
    nd = mods.pseudo_selection(cu(g['in0']), 0.8, 0.6, 'ndarray', -1)
    assert isinstance(nd, np.ndarray)
    with pytest.raises(AssertionError):
        mods.pseudo_selection(torch.full((1, 6, 4, 4), 1.5, device='cuda'), 0.8, 0.6, 'tensor', -1)


def test_pseudo_selection_full_size(mods):
    g = torch.Generator().manual_seed(5)
    soft = torch.softmax(torch.randn(8, 6, 512, 512, generator=g) * 3, 1)
    out = mods.pseudo_selection(soft.cuda(), 0.8, 0.6, 'tensor', -1).cpu().numpy()
    assert np.array_equal(out, olab.pseudo_selection(soft.numpy(), 0.8, 0.6, -1))


def test_downscale_and_prototypes_golden(mods, gold):
    g = gold('downscale.npz')
    ds = mods.DownscaleLabel(16, 6, -1, 0.75)(cu(g['lab'], torch.int64)).cpu().numpy()
    assert np.array_equal(ds, g['out'].astype(np.int64))
    g = gold('refine.npz')
    al = mods.Aligner(None, feat_channels=64, class_num=6, ignore_label=-1, decay=0.996)
    al.prototypes = cu(g['protos']).clone()
    ds = al.update_prototype(cu(g['feat_s']), cu(g['lab_s'], torch.int64))
    assert np.array_equal(ds.cpu().numpy(), g['ds'].astype(np.int64))
    # fp32 sums in a different order than the reference's (n,c,k) broadcast-sum: 1e-5 relative
    np.testing.assert_allclose(al.prototypes.cpu().numpy(), g['protos_new'], rtol=1e-5, atol=1e-6)


def test_label_refine_golden(mods, gold):
    g = gold('refine.npz')
    al = mods.Aligner(None, feat_channels=64, class_num=6, ignore_label=-1, decay=0.996)
    al.prototypes = cu(g['protos']).clone()
    out = al.label_refine(None, cu(g['feat_t']), [cu(g['p1']), cu(g['p2'])], cu(g['soft']), True, 'all', 2.0)
    # tolerance: fp32 with a different summation order in the k=64 Pearson contraction and fma
    # contraction in the interpolation; the 1/dist ~ 1e7 pixel saturates the softmax either way
    np.testing.assert_allclose(out.cpu().numpy(), g['out'], rtol=2e-4, atol=2e-6)


def test_label_refine_other_modes_golden(mods, gold):
    """Modes 'p' / 'l' / 'n' / 's' with label_t_sup=None and the single-tensor prediction branch
    (regda/gast/alignment.py:199,212-236,260-261) against outputs of the reference's own Aligner."""
    g = gold('refine.npz')
    al = mods.Aligner(None, feat_channels=64, class_num=6, ignore_label=-1, decay=0.996)
    al.prototypes = cu(g['protos']).clone()
    feat, p1, p2, soft = cu(g['feat_t']), cu(g['p1']), cu(g['p2']), cu(g['soft'])
    for key, preds, mode, temp in (('out_p', [p1, p2], 'p', 2.0), ('out_l', [p1, p2], 'l', 1.5), ('out_1', p1, 'all', 2.0)):
        out = al.label_refine(None, feat, preds, soft, True, mode, temp)
        np.testing.assert_allclose(out.cpu().numpy(), g[key], rtol=2e-4, atol=2e-6, err_msg=key)
    # a single tensor is the two-head kernel fed the same logits twice: bit-identical to passing it as a pair
    assert torch.equal(al.label_refine(None, feat, p1, soft, True, 'l', 2.0),
                       al.label_refine(None, feat, [p1, p1], soft, True, 'l', 2.0))
    for mode in ('n', 's'):
        assert al.label_refine(None, feat, [p1, p2], soft, True, mode, 2.0) is soft      # no view: returned as is
    assert al.label_refine(None, feat, [p1, p2], soft, False, 'all', 2.0) is soft


def test_label_refine_superpixel_view_golden(mods, gold):
    """label_refine with label_t_sup given (regda/gast/alignment.py:238-258), modes 'all' and 's', against outputs of the
    reference's own Aligner (make_goldens.gold_refine_sup; inputs shared with refine.npz): superpixels that do and do not
    fill a wave, single-pixel superpixels, and the batch's largest id (`ignored`) present in one image only."""
    g, gs = gold('refine.npz'), gold('refine_sup.npz')
    al = mods.Aligner(None, feat_channels=64, class_num=6, ignore_label=-1, decay=0.996)
    al.prototypes = cu(g['protos']).clone()
    feat, p1, p2, soft = cu(g['feat_t']), cu(g['p1']), cu(g['p2']), cu(g['soft'])
    sup = cu(gs['sup'].astype(np.int64), torch.int64).reshape(2, 1, 64, 64)
    for key, mode, temp in (('out_all', 'all', 2.0), ('out_s', 's', 1.5)):
        out = al.label_refine(sup, feat, [p1, p2], soft, True, mode, temp)
        np.testing.assert_allclose(out.cpu().numpy(), gs[key], rtol=2e-4, atol=2e-6, err_msg=key)
        cm = al._classmax_ws[:2 * 6 * 4].view(torch.float32).cpu().reshape(2, 6)
        assert torch.equal(cm, out.cpu().flatten(2).max(-1)[0])
    # mode 's' needs neither features nor predictions
    assert torch.equal(al.label_refine(sup, None, None, soft, True, 's', 1.5), al.label_refine(sup, feat, [p1, p2], soft, True, 's', 1.5))
    # modes 'p' / 'l' do not look at the superpixels, 'n' returns its input
    for mode in ('p', 'l'):
        assert torch.equal(al.label_refine(sup, feat, [p1, p2], soft, True, mode, 2.0),
                           al.label_refine(None, feat, [p1, p2], soft, True, mode, 2.0))
    assert al.label_refine(sup, feat, [p1, p2], soft, True, 'n', 2.0) is soft
    # an id outside the table: reported
    al.max_superpixels = 16
    with pytest.raises(ValueError):
        al.label_refine(sup, feat, [p1, p2], soft, True, 'all', 2.0)
    with pytest.raises(ValueError):
        al.label_refine(-sup - 1, feat, [p1, p2], soft, True, 's', 2.0)


def test_label_refine_superpixel_view_full_size_vs_oracle(mods):
    """2 x 6 x 512 x 512 with a SLIC-like map (a 16 x 16 grid of cells with ragged borders, ids up to 1088): the
    per-superpixel maxima are exact (a maximum has one answer), the rest carries the tolerance of the other views."""
    g = torch.Generator().manual_seed(12)
    b, k, h, w, H = 2, 256, 32, 32, 512
    feat = torch.randn(b, k, h, w, generator=g)
    protos = torch.randn(6, k, generator=g)
    p1, p2 = torch.randn(b, 6, h, w, generator=g) * 2, torch.randn(b, 6, h, w, generator=g) * 2
    soft = torch.softmax(torch.randn(b, 6, H, H, generator=g) * 3, 1)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(H), indexing='ij')
    jit = torch.randint(-3, 4, (b, H, H), generator=g)
    sup = (((yy + jit).clamp(0, H - 1) // 16) * 32 + (xx + jit.flip(-1)).clamp(0, H - 1) // 16).long()      # ids 0 .. 1023
    sup[1, 300:340, 100:200] = 1088                                          # the batch's largest id: ignored
    sup = sup.reshape(b, 1, H, H)
    al = mods.Aligner(None, feat_channels=k, class_num=6, ignore_label=-1, decay=0.996)
    al.prototypes = protos.cuda()
    for mode, temp in (('all', 2.0), ('s', 2.0)):
        ref = opath.label_refine(feat, protos, [p1, p2], soft, True, mode, temp, label_t_sup=sup)
        out = al.label_refine(sup.cuda(), feat.cuda(), [p1.cuda(), p2.cuda()], soft.cuda(), True, mode, temp).cpu()
        np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=5e-4, atol=1e-6, err_msg=mode)
    # the ignored superpixel keeps the weight of the other views: equal to the run without superpixels there
    plain = al.label_refine(None, feat.cuda(), [p1.cuda(), p2.cuda()], soft.cuda(), True, 'all', 2.0).cpu()
    withs = al.label_refine(sup.cuda(), feat.cuda(), [p1.cuda(), p2.cuda()], soft.cuda(), True, 'all', 2.0).cpu()
    ign = (sup == 1088).expand(-1, 6, -1, -1)
    assert torch.equal(plain[ign], withs[ign]) and not torch.equal(plain[~ign], withs[~ign])


def test_label_refine_full_size_vs_oracle(mods):
    g = torch.Generator().manual_seed(11)
    b, k, h, w = 2, 2048, 32, 32
    feat = torch.randn(b, k, h, w, generator=g)
    protos = torch.randn(6, k, generator=g)
    p1, p2 = torch.randn(b, 6, h, w, generator=g) * 2, torch.randn(b, 6, h, w, generator=g) * 2
    soft = torch.softmax(torch.randn(b, 6, 512, 512, generator=g) * 3, 1)
    ref = opath.label_refine(feat, protos, [p1, p2], soft)
    al = mods.Aligner(None, feat_channels=k, class_num=6, ignore_label=-1, decay=0.996)
    al.prototypes = protos.cuda()
    out = al.label_refine(None, feat.cuda(), [p1.cuda(), p2.cuda()], soft.cuda(), True, 'all', 2.0).cpu()
    # 1/dist amplifies the fp32 rounding of the 2048-term contraction (dist ~ 0.5 -> sim ~ 2):
    # stated tolerance 5e-4 relative on probabilities
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=5e-4, atol=1e-6)
    # the per-class maxima handed to pseudo_selection equal the maxima of the output
    cm = al._classmax_ws[:b * 6 * 4].view(torch.float32).cpu().reshape(b, 6)
    assert torch.equal(cm, out.flatten(2).max(-1)[0])


def test_loss_golden_and_grad(mods, gold):
    g = gold('loss.npz')
    p1, p2 = cu(g['p1']).requires_grad_(True), cu(g['p2']).requires_grad_(True)
    lab = cu(g['lab'], torch.int64)
    ce = mods.CrossEntropy(ignore_label=-1, class_balancer=None)
    loss = mods.loss_calc([p1, p2], lab, loss_fn=ce, multi=True)
    loss.backward()
    assert loss.item() == pytest.approx(float(g['loss']), rel=2e-6)
    np.testing.assert_allclose(p1.grad.cpu().numpy(), g['g1'], rtol=2e-4, atol=1e-8)
    np.testing.assert_allclose(p2.grad.cpu().numpy(), g['g2'], rtol=2e-4, atol=1e-8)
    cb = mods.ClassBalance(class_num=6, ignore_label=-1, decay=0.99, temperature=2.0)
    ceb = mods.CrossEntropy(ignore_label=-1, class_balancer=cb)
    q1, q2 = cu(g['p1']).requires_grad_(True), cu(g['p2']).requires_grad_(True)
    lossb = mods.loss_calc([q1, q2], lab, loss_fn=ceb, multi=True)
    lossb.backward()
    assert lossb.item() == pytest.approx(float(g['lossb']), rel=2e-6)
    np.testing.assert_allclose(cb.freq.cpu().numpy(), g['freq'], rtol=1e-6)
    np.testing.assert_allclose(q1.grad.cpu().numpy(), g['gb1'], rtol=2e-4, atol=1e-8)


def test_loss_full_size_vs_oracle(mods):
    g = torch.Generator().manual_seed(3)
    b = 4
    p1 = (torch.randn(b, 6, 32, 32, generator=g) * 2).requires_grad_(True)
    p2 = (torch.randn(b, 6, 32, 32, generator=g) * 2).requires_grad_(True)
    lab = torch.randint(-1, 6, (b, 512, 512), generator=g)
    ref = opath.loss_calc([p1, p2], lab, -1)
    ref.backward()
    q1, q2 = p1.detach().cuda().requires_grad_(True), p2.detach().cuda().requires_grad_(True)
    ce = mods.CrossEntropy(ignore_label=-1)
    loss = mods.loss_calc([q1, q2], lab.cuda(), loss_fn=ce, multi=True)
    loss.backward()
    assert loss.item() == pytest.approx(ref.item(), rel=1e-5)
    np.testing.assert_allclose(q1.grad.cpu().numpy(), p1.grad.numpy(), rtol=1e-3, atol=1e-9)
    np.testing.assert_allclose(q2.grad.cpu().numpy(), p2.grad.numpy(), rtol=1e-3, atol=1e-9)
    # single full-resolution prediction through CrossEntropy.forward (identity upsample)
    z = torch.randn(1, 6, 24, 40, generator=g)
    l2 = torch.randint(-1, 6, (1, 24, 40), generator=g)
    r2 = opath.cross_entropy_mean(z, l2, -1)
    assert ce(z.cuda(), l2.cuda()).item() == pytest.approx(r2.item(), rel=1e-5)


def test_teacher_probs_vs_oracle(mods):
    g = torch.Generator().manual_seed(8)
    p1, p2 = torch.randn(2, 6, 32, 32, generator=g) * 3, torch.randn(2, 6, 32, 32, generator=g) * 3
    ref = opath.teacher_probs(p1, p2, (512, 512))
    out = mods.ops.teacher_probs(p1.cuda(), p2.cuda(), (512, 512)).cpu()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-4, atol=1e-6)


def test_sam_region_map_assembly_bit_exact(mods, gold):
    """rgda_masks_to_regions (the reference's own part of SAM.get_local_regions, local_region_homog.py:51-56) against the
    region maps the reference loop produced, a ragged size against the oracle, and the `SAM` mirror around a stand-in
    mask generator."""
    from regda_amd import ops
    from regda_amd.utils.local_region_homog import SAM, regions_from_anns
    from oracle import regions as oreg
    g = gold('regions.npz')
    for i in range(int(g['n'])):
        masks, areas, thr = g[f'masks{i}'], g[f'areas{i}'], int(g[f'thr{i}'])
        out = ops.masks_to_regions(torch.from_numpy(masks).cuda(), torch.from_numpy(areas).cuda(), thr)
        assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), g[f'regions{i}']), i
    rng = np.random.default_rng(5)
    masks = (rng.random((37, 33, 17)) < 0.15).astype(np.uint8)             # 561 pixels: not a multiple of 16
    areas = masks.reshape(37, -1).sum(1).astype(np.int64)
    thr = int(np.median(areas))
    out = ops.masks_to_regions(torch.from_numpy(masks).cuda(), torch.from_numpy(areas).cuda(), thr)
    assert np.array_equal(out.cpu().numpy(), oreg.regions_from_masks(masks, areas, thr))
    big = (rng.random((250, 512, 512)) < 0.01).astype(np.uint8)            # a production-size case (250 masks, 512^2)
    big[3, 100:300, 50:400] = 1
    ab = big.reshape(250, -1).sum(1).astype(np.int64)
    out = ops.masks_to_regions(torch.from_numpy(big).cuda(), torch.from_numpy(ab).cuda(), 1024)
    assert np.array_equal(out.cpu().numpy(), oreg.regions_from_masks(big, ab, 1024))
    anns = [{'segmentation': masks[k].astype(bool), 'area': int(areas[k])} for k in range(37)]

    class Gen:
        def generate(self, image):
            assert image.shape == (33, 17, 3)
            return anns
    reg = SAM(Gen()).get_local_regions(np.zeros((33, 17, 3), np.uint8), area_thrshold=thr)
    assert reg.dtype == np.int32 and np.array_equal(reg, oreg.regions_from_masks(masks, areas, thr))
    assert int(regions_from_anns([], (8, 8)).abs().sum()) == 0


@pytest.mark.parametrize('shape,nreg,conf', [((8, 512, 512), 250, 3.0), ((2, 512, 512), 3000, 6.0), ((3, 100, 36), 60, 4.0), ((1, 4, 4), 2, 5.0)])
def test_fused_pseudo_selection_lrh_bit_exact(shape, nreg, conf):
    """rgda_pseudo_lrh (pseudo_selection + Homogenizer in one pass over the soft labels, the SSL step's chain:
    tools/train_ssl_reg.py:224-228) against the two entry points it replaces and against the oracle -- bit for bit, ties
    and region 0 included, at the golden sizes' scale and at the full 8 x 512 x 512."""
    from regda_amd import ops
    rng = np.random.default_rng(7)
    b, h, w = shape
    g = torch.Generator().manual_seed(11)
    blocks = torch.randn(b, 6, (h + 15) // 16, (w + 15) // 16, generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3)[:, :, :h, :w]
    soft = torch.softmax(conf * blocks + torch.randn(b, 6, h, w, generator=g), 1).contiguous()
    regs = np.zeros(shape, np.int64)
    for i in range(b):
        for r in range(1, nreg + 1):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            regs[i, y0:y0 + rng.integers(1, max(2, h // 4)), x0:x0 + rng.integers(1, max(2, w // 4))] = r
    sc, rc = soft.cuda(), torch.from_numpy(regs).cuda()
    cmax = sc.amax((2, 3)).contiguous()
    out, ws = ops.pseudo_lrh(sc, cmax, rc, 0.8, 0.6, 0.5, 6, -1, max_regions=4096)
    two = ops.lrh(ops.pseudo_select(sc, 0.8, 0.6, -1), rc, 0.5, 6, -1, max_regions=4096)
    assert torch.equal(out, two)
    hard = olab.pseudo_selection(soft.numpy(), 0.8, 0.6, -1)
    assert np.array_equal(out.cpu().numpy(), olab.homogenize(hard, regs, 0.5, 6, -1))
    if h * w >= 1024:
        assert 0.02 < float((out >= 0).float().mean()) < 0.98        # the case exercises both outcomes
    off = (b * 4096 * 7) * 4
    assert int(ws[off:off + 4].view(torch.int32).item()) == 0
    # a second call reuses the workspace (the counters and the histogram are cleared per call)
    out2, _ = ops.pseudo_lrh(sc, cmax, rc, 0.8, 0.6, 0.5, 6, -1, max_regions=4096, ws=ws)
    assert torch.equal(out2, out)


def test_fused_pseudo_selection_lrh_flags_and_limits():
    from regda_amd import ops
    soft = torch.softmax(4.0 * torch.randn(1, 6, 8, 8, generator=torch.Generator().manual_seed(0)), 1).cuda()
    regs = torch.zeros(1, 8, 8, dtype=torch.int64, device='cuda')
    regs[0, :4] = 9                                     # outside [0, max_regions = 8): left unchanged, flag bit 0
    regs[0, 4:, :4] = 3
    cmax = soft.amax((2, 3)).contiguous()
    out, ws = ops.pseudo_lrh(soft, cmax, regs, 0.8, 0.6, 0.5, 6, -1, max_regions=8)
    off = (1 * 8 * 7) * 4
    assert int(ws[off:off + 4].view(torch.int32).item()) & 1
    sel = ops.pseudo_select(soft, 0.8, 0.6, -1)
    assert torch.equal(out[0, :4], sel[0, :4])
    with pytest.raises(ValueError):                     # hw % 4 != 0: the two-call route serves it
        ops.pseudo_lrh(soft[:, :, :3, :3].contiguous(), cmax, regs[:, :3, :3].contiguous(), 0.8, 0.6, 0.5, 6, -1)
