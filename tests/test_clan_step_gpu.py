"""GPU: the category-level adversarial term of AlignStep (adv_kind='clan', regda_amd/gast/clan.py) at the small topology
and tile of test_adv_step_gpu.py (4 + 4 images of 128 x 128): with adv_weight = 0 nothing changes, bit for bit; with
adv_weight > 0 the two losses, the target rows of both heads' logit gradients and the discriminator after its Adam step
agree with the float64 restatement (tests/clan_ref.py) evaluated on the step's own logits; the preheat gives the plain BCE,
weight_grad=False drops exactly the weight map's part of the gradient; two runs are bit-identical; a saved run resumes bit
for bit.  The inputs of the restatement are the step's own logits, so the bounds cannot sit in the tolerance file: they
are formed here the same way, three times the bf16 storage model's deviation from float64 on those inputs plus the f32
floor of adv_ref (the longest accumulation of the chain, 16 * 8 ndf terms)."""
import os

import pytest
import torch

import clan_ref as C

R = C.R
pytestmark = pytest.mark.gpu
RT, NDF, ADV_W, EPS, LAM, SIZE = 'resnet17t', 32, 0.5, 0.4, 40.0, (128, 128)
FLOOR = 16 * 8 * NDF * R.U32


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
    from regda_amd.models.Discriminator import FCDiscriminator
    torch.manual_seed(seed)
    return FCDiscriminator(6, ndf=NDF).cuda()


def batch(seed=11):
    from regda_amd.synthetic import make_batch
    return {k: v.cuda() for k, v in make_batch(b=4, size=128, seed=seed, device='cpu').items()}


def new_step(model_seed=6, params=None, **kw):
    from regda_amd.align import AlignStep
    st = AlignStep(build(model_seed), torch.randn(6, 2048, generator=torch.Generator().manual_seed(1)), **kw)
    st.keep_debug = bool(kw.get('adv_weight'))
    st.adv.update(params or {})
    return st


def run(st, g, lr=1e-3):
    """one step -> what it left: the three returned losses, both adversarial losses, the debug tensors"""
    r = st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], lr)
    torch.cuda.synchronize()
    return dict(losses=[t.clone() for t in r], adv=st.loss_adv.clone(), disc=st.loss_disc.clone(), debug=dict(st.debug or {}))


def snapshot(d):
    return {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}


def final(st):
    f = dict(p=st.model.flat_p.clone(), mom=st.mom.clone(), protos=st.prototypes.clone())
    a = st.adv['aligner']
    if a is not None:
        f.update({'disc.' + k: p.detach().clone() for k, p in a.discriminators[0].named_parameters()})
        for i, s in enumerate(a.optimizer.state_dict()['state'].values()):
            f['adam%d.m' % i], f['adam%d.v' % i] = s['exp_avg'].clone(), s['exp_avg_sq'].clone()
        f['steps_done'] = torch.tensor(a.steps_done)
    return f


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def logits(debug):
    return [debug[k].cpu() for k in ('s1', 's2', 't1', 't2')]


def check_generator(out, before, weighted=True, weight_grad=True):
    """loss_adv and the target rows of both heads' logit gradients against the restatement on the step's own logits"""
    p = R.params64(before)
    s1, s2, t1, t2 = logits(out['debug'])
    gen = {sto: C.generator_term(p, t1, t2, SIZE, ADV_W, 0, EPS, LAM, weighted, weight_grad, storage=sto) for sto in (False, True)}
    for i in (1, 2):
        bound = 3 * R.rel2(gen[True]['dx%d' % i], gen[False]['dx%d' % i]) + FLOOR
        e = R.rel2(out['debug']['g%d_t' % i].cpu(), gen[False]['dx%d' % i])
        print('[clan step] head %d target logit gradient rel2 %.3e bound %.3e' % (i, e, bound))
        assert e < bound, (i, e, bound)
    want = float(gen[False]['loss'])
    bound = 3 * abs(float(gen[True]['loss']) - want) + FLOOR * abs(want)
    print('[clan step] loss_adv %.7g ref %.7g (+- %.2e)' % (out['adv'].item(), want, bound))
    assert abs(out['adv'].item() - want) < bound
    return gen[False]


def check_discriminator(out, before, d, weighted=True, first_step=True):
    """loss_disc and the discriminator's gradients; on Adam's first step (zero moments) also where the parameters moved"""
    p = R.params64(before)
    s1, s2, t1, t2 = logits(out['debug'])
    dis = {sto: C.discriminator_term(p, (s1, s2), (t1, t2), SIZE, 0, 1, EPS, LAM, weighted, storage=sto) for sto in (False, True)}
    want = float(dis[False]['loss'])
    bound = 3 * abs(float(dis[True]['loss']) - want) + FLOOR * abs(want)
    print('[clan step] loss_disc %.7g ref %.7g (+- %.2e)' % (out['disc'].item(), want, bound))
    assert abs(out['disc'].item() - want) < bound
    for k in R.PARAMS:
        g_ref, q = dis[False]['grads'][k], d.get_parameter(k)
        bound = 3 * R.rel2(dis[True]['grads'][k], g_ref) + FLOOR
        e = R.rel2(q.grad.cpu(), g_ref)
        n, most = R.opposite(q.detach().cpu() - before[k], -g_ref), R.opposite_bound(dis[True]['grads'][k], g_ref)
        print('[clan step] %s gradient rel2 %.3e bound %.3e; adam: %d of %d elements move against the restatement, bound %d'
              % (k, e, bound, n, g_ref.numel(), most))
        assert e < bound, (k, e, bound)
        if first_step:
            assert R.adam_first_step_check(before[k], q, q.grad), k
            assert n <= most, (k, n, most)


@pytest.fixture(scope='module')
def g():
    return batch()


@pytest.fixture(scope='module')
def clan_run(g):
    d = discriminator()
    before = snapshot(d)
    st = new_step(adv_weight=ADV_W, adv_kind='clan', discriminators=[d])
    return st, run(st, g), d, before


def test_one_step_matches_the_restatement_on_its_own_logits(clan_run):
    st, out, d, before = clan_run
    from regda_amd.gast.clan import CategoryAdversarialAligner
    a = st.adv['aligner']
    assert isinstance(a, CategoryAdversarialAligner) and a.discriminators == [d] and a.steps_done == 1
    assert st.adv['kind'] == 'clan' and (a.epsilon, a.lambda_local, a.preheat_steps, a.weight_grad) == (EPS, LAM, 0, True)
    check_generator(out, before)
    check_discriminator(out, before, d)


def test_two_runs_are_bit_identical(clan_run, g):
    st, out, d, before = clan_run
    st2 = new_step(adv_weight=ADV_W, adv_kind='clan', discriminators=[discriminator()])
    out2 = run(st2, g)
    assert all(torch.equal(a, b) for a, b in zip(out['losses'], out2['losses']))
    assert torch.equal(out['adv'], out2['adv']) and torch.equal(out['disc'], out2['disc'])
    same(out['debug'], out2['debug'])
    same(final(st), final(st2))


def test_zero_weight_is_bit_identical_to_a_step_without_the_arguments(g):
    st0, st1 = new_step(), new_step(adv_kind='clan', adv_weight=0.0)
    out0, out1 = run(st0, g), run(st1, g)
    assert st1.adv['aligner'] is None and st1.adv['kind'] == 'clan' and out1['adv'].item() == 0.0 and out1['disc'].item() == 0.0
    assert all(torch.equal(a, b) for a, b in zip(out0['losses'], out1['losses']))
    same(final(st0), final(st1))


def test_preheat_gives_the_plain_loss_then_the_weighted_one(clan_run, g):
    """preheat_steps = 1: step 0 is the plain BCE on the upsampled map on both sides, step 1 the weighted loss; each against
    the restatement on that step's logits and the discriminator as it stood before that step"""
    d = discriminator()
    st = new_step(adv_weight=ADV_W, adv_kind='clan', discriminators=[d], params=dict(preheat_steps=1))
    before = snapshot(d)
    out = run(st, g)
    assert st.adv['aligner'].steps_done == 1 and st.adv['aligner'].preheat_steps == 1
    plain = check_generator(out, before, weighted=False)
    check_discriminator(out, before, d, weighted=False)
    # the model saw no weight map yet: up to here the step differs from the fixture's in the adversarial term alone
    same({k: out['debug'][k] for k in ('s1', 's2', 't1', 't2')}, {k: clan_run[1]['debug'][k] for k in ('s1', 's2', 't1', 't2')})
    weighted = C.generator_term(R.params64(before), *logits(out['debug'])[2:], SIZE, ADV_W, 0, EPS, LAM)
    assert abs(float(weighted['loss'] - plain['loss'])) > 0.05 * abs(float(plain['loss'])), 'the two losses are told apart'
    before = snapshot(d)
    out = run(st, batch(12))
    assert st.adv['aligner'].steps_done == 2
    check_generator(out, before, weighted=True)
    check_discriminator(out, before, d, weighted=True, first_step=False)


def test_weight_grad_false_drops_exactly_the_weight_maps_part(clan_run, g):
    st, out, d, before = clan_run
    d2 = discriminator()
    st2 = new_step(adv_weight=ADV_W, adv_kind='clan', discriminators=[d2], params=dict(weight_grad=False))
    out2 = run(st2, g)
    assert st2.adv['aligner'].weight_grad is False
    same({k: out['debug'][k] for k in ('s1', 's2', 't1', 't2')}, {k: out2['debug'][k] for k in ('s1', 's2', 't1', 't2')})
    assert torch.equal(out['adv'], out2['adv']), 'the loss itself does not change'
    check_generator(out2, before, weight_grad=False)
    # the difference of the two steps' gradients is the weight map's part: the restatement's, within the bounds of both
    p = R.params64(before)
    t1, t2 = logits(out['debug'])[2:]
    ref = {wg: C.generator_term(p, t1, t2, SIZE, ADV_W, 0, EPS, LAM, True, wg) for wg in (True, False)}
    sto = {wg: C.generator_term(p, t1, t2, SIZE, ADV_W, 0, EPS, LAM, True, wg, storage=True) for wg in (True, False)}
    for i in (1, 2):
        k = 'dx%d' % i
        part = ref[True][k] - ref[False][k]
        assert float(part.norm()) > 0.01 * float(ref[True][k].norm()), 'the weight map carries a visible part of the gradient'
        got = out['debug']['g%d_t' % i].double().cpu() - out2['debug']['g%d_t' % i].double().cpu()
        bound = sum(3 * float((sto[wg][k] - ref[wg][k]).norm()) + FLOOR * float(ref[wg][k].norm()) for wg in (True, False))
        e = float((got - part).norm())
        print('[clan step] head %d weight-map part of the gradient: |diff| %.3e bound %.3e (|part| %.3e)' % (
            i, e, bound, float(part.norm())))
        assert e < bound


def test_a_saved_run_resumes_bit_for_bit(g, tmp_path):
    from regda_amd.checkpoint import load_training_state, save_training_state
    batches = [g, batch(12)]
    params = dict(preheat_steps=1, lambda_local=10.0)

    def fresh(model_seed=6, disc_seed=77, params=params):
        return new_step(model_seed, params, adv_weight=ADV_W, adv_kind='clan', discriminators=[discriminator(disc_seed)])

    a = fresh()
    A = [run(a, b) for b in batches]
    b = fresh()
    run(b, batches[0])
    path = os.path.join(tmp_path, 'clan.pth')
    save_training_state(path, b, 1)
    sd = torch.load(path, weights_only=True)['step']
    assert sd['adv']['clan'] == dict(steps_done=1, epsilon=EPS, lambda_local=10.0, preheat_steps=1)
    assert set(sd['adv']) == {'discriminators', 'optimizer', 'clan'} and len(sd['adv']['discriminators']) == 1
    c = fresh(model_seed=9, disc_seed=5, params=None)
    assert c.adv['aligner'].steps_done == 0 and c.adv['lambda_local'] == LAM
    assert load_training_state(path, c) == 1
    assert c.adv['aligner'].steps_done == 1 and c.adv['lambda_local'] == 10.0 and c.adv['preheat_steps'] == 1
    out = run(c, batches[1])
    assert all(torch.equal(x, y) for x, y in zip(A[1]['losses'], out['losses']))
    assert torch.equal(A[1]['adv'], out['adv']) and torch.equal(A[1]['disc'], out['disc'])
    same(final(a), final(c))
    # the entry is validated before anything is written
    kept = final(c)
    for bad, match in ((dict(sd['adv']['clan'], steps_done=-1), 'steps_done'), (dict(sd['adv']['clan'], epsilon='x'), 'epsilon'),
                       ({k: v for k, v in sd['adv']['clan'].items() if k != 'preheat_steps'}, 'preheat_steps')):
        with pytest.raises(ValueError, match=match):
            c.load_state_dict(dict(sd, adv=dict(sd['adv'], clan=bad)))
    with pytest.raises(ValueError, match='clan'):
        c.load_state_dict(dict(sd, adv={k: v for k, v in sd['adv'].items() if k != 'clan'}))
    same(kept, final(c))
    # the plain aligner's state gains no key
    from regda_amd.gast.adversarial import AdversarialAligner
    assert set(AdversarialAligner([discriminator()]).state_dict()) == {'discriminators', 'optimizer'}


def test_refusals(clan_run, g):
    from regda_amd.align import AlignStep
    st = clan_run[0]
    protos = torch.randn(6, 2048)
    with pytest.raises(ValueError, match='one discriminator'):
        AlignStep(build(), protos, adv_weight=ADV_W, adv_kind='clan', discriminators=[discriminator(), discriminator()])
    with pytest.raises(ValueError, match='one discriminator'):
        AlignStep(build(), protos, adv_weight=ADV_W, adv_kind='clan', discriminators=[None, None])
    one = AlignStep(build(), protos, adv_weight=ADV_W, adv_kind='clan', discriminators=[None, discriminator()])
    assert len(one.adv['aligner'].discriminators) == 1
    made = AlignStep(build(), protos, adv_weight=ADV_W, adv_kind='clan')
    assert made.adv['aligner'].discriminators[0].num_classes == 6
    # step.adv is the step's only source of the CLAN parameters: checked before anything is launched, at every step
    kept = final(st)
    for key, bad in (('epsilon', -0.1), ('lambda_local', float('nan')), ('preheat_steps', 1.5), ('preheat_steps', -1)):
        good, st.adv[key] = st.adv[key], bad
        try:
            with pytest.raises(ValueError, match=key):
                st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], 1e-3)
        finally:
            st.adv[key] = good
    same(kept, final(st))
    st.reducer.force = True             # what data-parallel ranks (or RGDA_FORCE_DDP) make of `reducer.active`
    try:
        with pytest.raises(NotImplementedError, match='all-reduced'):
            st.step(g['images_s'], g['label_s'], g['images_t'], g['regs_t'], 1e-3)
    finally:
        st.reducer.force = False
