"""GPU: the adversarial term of AlignStep (regda_amd/gast/adversarial.py) at the smallest batch and tile test_align_gpu.py
uses (4 + 4 images of 128 x 128, the shallow topology): adv_weight = 0 changes nothing, bit for bit; with adv_weight > 0
the two losses, the target rows of the logit gradients and the discriminators after their Adam step agree with the float64
restatement (tests/adv_ref.py) evaluated on the step's own logits; two runs are bit-identical; data-parallel ranks and
the SSL step refuse.  The inputs of the restatement are the step's own logits, so the bounds cannot sit in the tolerance
file: they are formed here the same way, three times the bf16 storage model's deviation from float64 on those inputs plus
the f32 floor of adv_ref."""
import pytest
import torch

import adv_ref as R

pytestmark = pytest.mark.gpu
RT, NDF, ADV_W, HEAD_W = 'resnet17t', 32, 0.5, (1.0, 0.25)


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


def discriminators():
    from regda_amd.models.Discriminator import FCDiscriminator
    torch.manual_seed(77)
    return [FCDiscriminator(6, ndf=NDF).cuda() for _ in range(2)]


def one_step(**kw):
    from regda_amd.align import AlignStep
    from regda_amd.synthetic import make_batch
    m = build()
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(1))
    st = AlignStep(m, protos, **kw)
    st.keep_debug = bool(kw.get('adv_weight'))
    if kw.get('adv_weight'):
        st.adv['head_weights'] = HEAD_W
    g = {k: v.cuda() for k, v in make_batch(b=4, size=128, seed=11, device='cpu').items()}
    lseg, lal, gn = st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], 1e-3)
    torch.cuda.synchronize()
    return st, m, (lseg.clone(), lal.clone(), gn.clone())


def test_zero_weight_is_bit_identical_to_a_step_without_the_argument():
    st0, m0, l0 = one_step()
    st1, m1, l1 = one_step(adv_weight=0.0)
    assert st1.adv['aligner'] is None and st1.loss_adv.item() == 0.0 and st1.loss_disc.item() == 0.0
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    for (k, a), (_, b) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(a, b), k
    assert torch.equal(st0.prototypes, st1.prototypes)


@pytest.fixture(scope='module')
def adv_run():
    ds = discriminators()
    before = [{k: v.detach().cpu().clone() for k, v in d.state_dict().items()} for d in ds]
    st, m, losses = one_step(adv_weight=ADV_W, discriminators=ds)
    return st, m, losses, ds, before


def test_terms_match_the_restatement_on_the_steps_own_logits(adv_run):
    st, m, losses, ds, before = adv_run
    size = (128, 128)
    loss_adv = loss_disc = 0.0
    tol_adv = tol_disc = 0.0
    for i, d in enumerate(ds):
        w = ADV_W * HEAD_W[i]
        p = R.params64(before[i])
        xs, xt = st.debug['s%d' % (i + 1)].cpu(), st.debug['t%d' % (i + 1)].cpu()
        Ps, Pt = R.probs(xs, size), R.probs(xt, size)
        # generator term: BCE against the source label through the target probabilities, the input gradient only
        gen = {sto: R.disc_loss_grads(p, Pt, 0, storage=sto, scale=w) for sto in (False, True)}
        dlogits = {sto: R.probs_backward(xt, gen[sto]['dx'], size) for sto in (False, True)}
        floor = 16 * 8 * NDF * R.U32
        bound = 3 * R.rel2(dlogits[True], dlogits[False]) + floor
        e = R.rel2(st.debug['g%d_t' % (i + 1)].cpu(), dlogits[False])
        print('[adv step head %d] target logit gradient rel2 %.3e bound %.3e' % (i, e, bound))
        assert e < bound
        loss_adv += float(gen[False]['loss'])
        tol_adv += 3 * abs(float(gen[True]['loss'] - gen[False]['loss'])) + floor * abs(float(gen[False]['loss']))
        # discriminator step: 0.5 * (BCE(D(P_s), 0) + BCE(D(P_t), 1)), Adam on the summed gradients
        dis = {sto: (R.disc_loss_grads(p, Ps, 0, storage=sto, scale=0.5), R.disc_loss_grads(p, Pt, 1, storage=sto, scale=0.5))
               for sto in (False, True)}
        total = {sto: {k: dis[sto][0]['grads'][k] + dis[sto][1]['grads'][k] for k in R.PARAMS} for sto in (False, True)}
        loss_disc += float(dis[False][0]['loss'] + dis[False][1]['loss'])
        tol_disc += 3 * abs(float(dis[True][0]['loss'] + dis[True][1]['loss'] - dis[False][0]['loss'] - dis[False][1]['loss'])) \
            + floor * abs(float(dis[False][0]['loss'] + dis[False][1]['loss']))
        for k in R.PARAMS:
            g_ref = total[False][k]
            bound = 3 * R.rel2(total[True][k], g_ref) + floor
            e = R.rel2(d.get_parameter(k).grad.cpu(), g_ref)
            q = d.get_parameter(k)
            n, most = R.opposite(q.detach().cpu() - before[i][k], -g_ref), R.opposite_bound(total[True][k], g_ref)
            print('[adv step head %d] %s gradient rel2 %.3e bound %.3e; adam: %d of %d elements move against the restatement, '
                  'bound %d' % (i, k, e, bound, n, g_ref.numel(), most))
            assert e < bound, (i, k, e, bound)
            assert R.adam_first_step_check(before[i][k], q, q.grad), (i, k)
            assert n <= most, (i, k, n, most)
    print('[adv step] loss_adv %.7g ref %.7g (+- %.2e)  loss_disc %.7g ref %.7g (+- %.2e)' % (
        st.loss_adv.item(), loss_adv, tol_adv, st.loss_disc.item(), loss_disc, tol_disc))
    assert abs(st.loss_adv.item() - loss_adv) < tol_adv
    assert abs(st.loss_disc.item() - loss_disc) < tol_disc


def test_two_runs_are_bit_identical(adv_run):
    st, m, losses, ds, before = adv_run
    ds2 = discriminators()
    st2, m2, losses2 = one_step(adv_weight=ADV_W, discriminators=ds2)
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))
    assert torch.equal(st.loss_adv, st2.loss_adv) and torch.equal(st.loss_disc, st2.loss_disc)
    for d, d2 in zip(ds, ds2):
        for (k, a), (_, b) in zip(d.named_parameters(), d2.named_parameters()):
            assert torch.equal(a, b), k
    for (k, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k


def test_refusals(adv_run):
    from regda_amd.align import AlignStep
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    st = adv_run[0]
    g = {k: v.cuda() for k, v in make_batch(b=4, size=128, seed=11, device='cpu').items()}
    st.reducer.force = True             # what data-parallel ranks (or RGDA_FORCE_DDP) make of `reducer.active`
    try:
        with pytest.raises(NotImplementedError, match='all-reduced'):
            st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], 1e-3)
    finally:
        st.reducer.force = False
    protos = torch.randn(6, 2048)
    with pytest.raises(NotImplementedError, match='AlignStep'):
        SSLStep(build(), protos, adv_weight=0.1)
    with pytest.raises(ValueError, match='adv_weight'):
        AlignStep(build(), protos, adv_weight=-1.0)
