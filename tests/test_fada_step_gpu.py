"""GPU: the feature-adversarial term of SourceStep (regda_amd/gast/fada.py) at the batch and tile test_adv_step_gpu.py
uses (4 + 4 images of 128 x 128, the shallow topology: 8 x 8 feature pixels), ndf = 64: fada_weight = 0 changes nothing, bit
for bit; with the weight on the two losses, the target gradient rows and the discriminator after its Adam step agree with
the float64 restatement (tests/fada_ref.py) evaluated on the step's own features and logits; with align_domain as well the
CORAL loss keeps its bits; two runs are bit-identical; a saved and resumed run continues with the bits of the uninterrupted
one; data-parallel ranks refuse.  The inputs of the restatement are the step's own tensors, so the bounds cannot sit in the
tolerance file: they are formed here the same way, three times the bf16 storage model's deviation from float64 on those
inputs plus the f32 floor (the longest accumulation, 9 * 2048 terms)."""
import pytest
import torch

import fada_ref as R

pytestmark = pytest.mark.gpu
RT, NDF, FADA_W = 'resnet17t', 64, 0.5
FLOOR = 9 * 2048 * R.U32


def build(seed=6):
    from oracle import model as omodel
    from regda_amd.models.Encoder import Deeplabv2
    sd = omodel.init_state_dict(RT, 6, seed=seed)
    m = Deeplabv2(dict(backbone=dict(resnet_type=RT, output_stride=16, pretrained=False), multi_layer=True, cascade=False,
                       use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048, num_classes=6,
                       is_ins_norm=True))
    m.load_state_dict(sd, strict=True)
    ones = torch.ones(4, 512)
    m.set_drop_masks(ones, ones)
    return m


def discriminator(seed=77):
    from regda_amd.models.PixelDiscriminator import PixelDiscriminator
    torch.manual_seed(seed)
    return PixelDiscriminator(2048, NDF, 6).cuda()


def batch(seed=11):
    from regda_amd.synthetic import make_batch
    return {k: v.cuda() for k, v in make_batch(b=4, size=128, seed=seed, device='cpu').items()}


def make_step(**kw):
    from regda_amd.source import SourceStep
    m = build()
    st = SourceStep(m, **kw)
    st.keep_debug = bool(kw.get('fada_weight'))
    return st, m


def run(st, seed=11):
    g = batch(seed)
    out = st.step(g['images_s'], g['label_s'], g['images_t'], 1e-3)
    torch.cuda.synchronize()
    return tuple(t.clone() for t in out)


def same_model(m0, m1):
    for (k, a), (_, b) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(a, b), k
    for (k, a), (_, b) in zip(m0.named_buffers(), m1.named_buffers()):
        assert torch.equal(a, b), k


def same_discriminator(d0, d1):
    for (k, a), (_, b) in zip(d0.named_parameters(), d1.named_parameters()):
        assert torch.equal(a, b), k


def test_zero_weight_is_bit_identical_to_a_step_without_the_argument():
    st0, m0 = make_step()
    st1, m1 = make_step(fada_weight=0.0)
    l0, l1 = run(st0), run(st1)
    assert st1.fada['aligner'] is None and st1.loss_fada.item() == 0.0 and st1.loss_fada_disc.item() == 0.0
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    same_model(m0, m1)


@pytest.fixture(scope='module')
def fada_run():
    d = discriminator()
    before = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}
    st, m = make_step(fada_weight=FADA_W, pixel_discriminator=d)
    losses = run(st)
    return st, m, losses, d, before


def nchw_rows(rows, like):
    b, _, h, w = like.shape
    return R.nchw(rows.detach().cpu().to(R.F64), b, h, w)


def check_generator(st, before, tag):
    p = R.params64(before)
    feat_t, t2 = st.debug['feat_t'].cpu(), st.debug['t2'].cpu()
    assert feat_t.shape == (4, 2048, 8, 8) and t2.shape == (4, 6, 8, 8)
    onto = nchw_rows(st.debug['rows_t_before'], feat_t)
    gen = {sto: R.disc_loss_grads(p, feat_t, t2, 0, scale=FADA_W, storage=sto, onto=onto) for sto in (False, True)}
    bound = 3 * R.rel2(gen[True]['dx'], gen[False]['dx']) + FLOOR
    e = R.rel2(nchw_rows(st.debug['rows_t'], feat_t), gen[False]['dx'])
    ref = float(gen[False]['loss'])
    tol = 3 * abs(float(gen[True]['loss']) - ref) + FLOOR * abs(ref)
    print('[fada step %s] target rows rel2 %.3e bound %.3e; loss_fada %.7g ref %.7g (+- %.2e)' % (
        tag, e, bound, st.loss_fada.item(), ref, tol))
    assert e < bound
    assert abs(st.loss_fada.item() - ref) < tol


def test_terms_match_the_restatement_on_the_steps_own_tensors(fada_run):
    st, m, losses, d, before = fada_run
    assert not bool(st.debug['rows_t_before'].any())            # no domain term: the rows start at zero
    check_generator(st, before, 'fada only')
    p = R.params64(before)
    dbg = {k: v.cpu() for k, v in st.debug.items()}
    dis = {sto: (R.disc_loss_grads(p, dbg['feat_s'], dbg['s2'], 0, scale=0.5, storage=sto),
                 R.disc_loss_grads(p, dbg['feat_t'], dbg['t2'], 1, scale=0.5, storage=sto)) for sto in (False, True)}
    total = {sto: {k: dis[sto][0]['grads'][k] + dis[sto][1]['grads'][k] for k in R.PARAMS} for sto in (False, True)}
    loss = {sto: float(dis[sto][0]['loss'] + dis[sto][1]['loss']) for sto in (False, True)}
    tol = 3 * abs(loss[True] - loss[False]) + FLOOR * abs(loss[False])
    print('[fada step] loss_fada_disc %.7g ref %.7g (+- %.2e)' % (st.loss_fada_disc.item(), loss[False], tol))
    assert abs(st.loss_fada_disc.item() - loss[False]) < tol
    for k in R.PARAMS:
        g_ref = total[False][k]
        bound = 3 * R.rel2(total[True][k], g_ref) + FLOOR
        q = d.get_parameter(k)
        e = R.rel2(q.grad.cpu(), g_ref)
        n, most = R.opposite(q.detach().cpu() - before[k], -g_ref), R.opposite_bound(total[True][k], g_ref)
        print('[fada step] %s gradient rel2 %.3e bound %.3e; adam: %d of %d elements move against the restatement, bound %d'
              % (k, e, bound, n, g_ref.numel(), most))
        assert e < bound, (k, e, bound)
        assert R.adam_first_step_check(before[k], q, q.grad), k
        assert n <= most, (k, n, most)


def test_coral_keeps_its_bits_next_to_the_term():
    st_c, _ = make_step(align_domain=True)
    lc = run(st_c)
    d = discriminator()
    before = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}
    st, _ = make_step(align_domain=True, fada_weight=FADA_W, pixel_discriminator=d)
    l = run(st)
    assert torch.equal(lc[1], l[1]) and torch.equal(lc[0], l[0])          # CORAL and the segmentation loss, bit for bit
    assert bool(st.debug['rows_t_before'].any())
    check_generator(st, before, 'after CORAL')


def test_two_runs_are_bit_identical(fada_run):
    st, m, losses, d, before = fada_run
    d2 = discriminator()
    st2, m2 = make_step(fada_weight=FADA_W, pixel_discriminator=d2)
    losses2 = run(st2)
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))
    assert torch.equal(st.loss_fada, st2.loss_fada) and torch.equal(st.loss_fada_disc, st2.loss_fada_disc)
    same_discriminator(d, d2)
    same_model(m, m2)


def test_resume_continues_with_the_bits_of_the_uninterrupted_run():
    d = discriminator()
    st, m = make_step(fada_weight=FADA_W, pixel_discriminator=d)
    run(st, 11)
    sd = st.state_dict()
    assert 'fada' in sd and set(sd['fada']) == {'discriminator', 'optimizer'}
    second = run(st, 12)
    d2 = discriminator(seed=5)              # another initialisation: everything comes from the state
    st2, m2 = make_step(fada_weight=FADA_W, pixel_discriminator=d2)
    st2.load_state_dict(sd)
    resumed = run(st2, 12)
    assert all(torch.equal(a, b) for a, b in zip(second, resumed))
    assert torch.equal(st.loss_fada, st2.loss_fada) and torch.equal(st.loss_fada_disc, st2.loss_fada_disc)
    same_discriminator(d, d2)
    same_model(m, m2)
    st3, _ = make_step()
    with pytest.raises(ValueError, match='step.fada'):
        st3.load_state_dict(sd)


def test_refusals(fada_run):
    st = fada_run[0]
    g = batch()
    with pytest.raises(ValueError, match='target images'):
        st.step(g['images_s'], g['label_s'], None, 1e-3)
    st.reducer.force = True             # what data-parallel ranks (or RGDA_FORCE_DDP) make of `reducer.active`
    try:
        with pytest.raises(NotImplementedError, match='all-reduced'):
            st.step(g['images_s'], g['label_s'], g['images_t'], 1e-3)
    finally:
        st.reducer.force = False
    st.fada['temperature'] = 0.0        # read at every step, refused before the forward
    try:
        with pytest.raises(ValueError, match='temperature'):
            st.step(g['images_s'], g['label_s'], g['images_t'], 1e-3)
    finally:
        st.fada['temperature'] = 1.8
    with pytest.raises(NotImplementedError):
        st.capture()
    with pytest.raises(NotImplementedError):
        st.record_plan()
    st0, _ = make_step()
    st0.fada_weight = 0.5
    with pytest.raises(ValueError, match='aligner'):
        st0.step(g['images_s'], g['label_s'], g['images_t'], 1e-3)
