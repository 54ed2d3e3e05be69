"""GPU: a run that is stopped, saved (regda_amd/checkpoint.py) and resumed in a FRESH model and step -- built from
another initialisation, other prototypes and another generator seed -- continues with the bits of the uninterrupted
run.  Every step is bit-reproducible (tests/test_determinism_gpu.py), so every comparison here is torch.equal against
the uninterrupted run of the same code; there is no tolerance anywhere.

Shapes are those of tests/test_determinism_gpu.py: the shallow resnet17t topology, 2 + 2 tiles of 128 x 128."""
import os

import pytest
import torch

from oracle import model as omodel

pytestmark = pytest.mark.gpu

RT = 'resnet17t'
LRS = [1e-3, 2e-3, 1e-3, 3e-3]


def build(C=6, use_ppm=True):
    from regda_amd.models.Encoder import Deeplabv2
    return Deeplabv2(dict(backbone=dict(resnet_type=RT, output_stride=16, pretrained=False), multi_layer=True,
                          cascade=False, use_ppm=use_ppm, ppm=dict(num_classes=C, use_aux=False, fc_dim=2048),
                          inchannels=2048, num_classes=C, is_ins_norm=True))


_INIT = {}


def init_sd(seed):
    """the oracle's initial weights of a seed: made once, shared, never written"""
    if seed not in _INIT:
        _INIT[seed] = omodel.init_state_dict(RT, 6, seed=seed)
    return _INIT[seed]


def protos(seed, C=6):
    return torch.randn(C, 2048, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope='module')
def batches():
    from regda_amd.synthetic import make_batch
    b1, b2 = make_batch(b=2, size=128, seed=21), make_batch(b=2, size=128, seed=22)
    return [b1, b2, b1, b2]


# ---------------------------------------------------------------------------------------------------------------- SSL
def ssl_step(cfg, init_seed=12, torch_seed=77, proto_seed=5):
    """A fresh model and SSL step.  cfg 'online': EMA teacher (ema_decay=0.9), plain CE; 'offline': offline soft labels,
    both ClassBalances, loss_t='gdp'; 'plain': offline soft labels, nothing else.  The resumed runs are built with other
    seeds throughout: whatever they need must come out of the saved state."""
    from regda_amd.gast.balance import ClassBalance
    from regda_amd.ssl import SSLStep
    m = build()
    m.load_state_dict(init_sd(init_seed), strict=True)
    torch.manual_seed(torch_seed)            # Dropout2d seeds come from the global CPU generator
    kw = dict(ema_decay=0.9)
    if cfg == 'offline':
        kw = dict(class_balancer_s=ClassBalance(class_num=6, ignore_label=-1, decay=0.99, temperature=0.5),
                  class_balancer_t=ClassBalance(class_num=6, ignore_label=-1, decay=0.99, temperature=0.5), loss_t='gdp')
    elif cfg == 'plain':
        kw = {}
    return SSLStep(m, protos(proto_seed), **kw)


def ssl_steps(st, cfg, batches, which, record_at=None):
    """Run the steps `which` of the sequence -> per step what it returned and left behind, cloned"""
    out = []
    for i in which:
        b = batches[i]
        args = (b['images_s'], b['label_s'], b['images_t'], None if cfg == 'online' else b['soft_t'], b['regs_t'])
        if i == record_at:
            st.record_plan(*args, lr=LRS[i])
            r = st._out
        else:
            r = st.step(*args, LRS[i])
        out.append(dict(loss_s=r[0].clone(), loss_t=r[1].clone(), gn=r[2].clone(), hard=st.last_hard.clone(),
                        soft=st.last_soft_t.clone(), p=st.model.flat_p.clone()))
    torch.cuda.synchronize()
    return out


def ssl_final(st):
    torch.cuda.synchronize()
    f = dict(p=st.model.flat_p.clone(), buf=st.model.flat_buf.clone(), nbt=st.model.flat_nbt.clone(), mom=st.mom.clone(),
             protos=st.prototypes.clone())
    if st.teacher is not None:
        f['shadow'] = st.teacher.flat_p.clone()
    for name in ('class_balancer_s', 'class_balancer_t'):
        if getattr(st, name) is not None:
            f[name] = getattr(st, name).freq.clone()
    if st.loss_fn_t.kind == 'gdp':
        f.update(acc_sum=st.loss_fn_t.acc_sum.clone(), bins_weight=st.loss_fn_t.bins_weight.clone())
    return f


def assert_same(ref_steps, ref_final, steps, final, what):
    assert len(ref_steps) == len(steps)
    for i, (x, y) in enumerate(zip(ref_steps, steps)):
        for k in x:
            assert torch.equal(x[k], y[k]), f'{what}: step {i} of the continuation: {k} differs'
    assert set(ref_final) == set(final)
    for k in ref_final:
        assert torch.equal(ref_final[k], final[k]), f'{what}: final {k} differs ' \
            f'({(ref_final[k] != final[k]).sum().item()} of {ref_final[k].numel()} elements)'


_CACHE = {}


def uninterrupted(cfg, batches, tmp_dir):
    """Per configuration, computed once and shared: run A (four steps, uninterrupted) and the file run B saved after two
    steps of the same run."""
    if cfg not in _CACHE:
        from regda_amd.checkpoint import save_training_state
        a = ssl_step(cfg)
        steps = ssl_steps(a, cfg, batches, range(4))
        b = ssl_step(cfg)
        first_two = ssl_steps(b, cfg, batches, range(2))
        for x, y in zip(steps, first_two):
            assert all(torch.equal(x[k], y[k]) for k in x)
        path = os.path.join(tmp_dir, f'ssl_{cfg}.pth')
        save_training_state(path, b, 2)
        assert len({float(s['loss_s']) for s in steps}) == 4        # the steps did train
        _CACHE[cfg] = dict(steps=steps, final=ssl_final(a), path=path)
    return _CACHE[cfg]


@pytest.fixture(scope='module')
def tmp_dir(tmp_path_factory):
    yield str(tmp_path_factory.mktemp('resume'))
    _CACHE.clear()


@pytest.mark.parametrize('cfg', ['online', 'offline'])
def test_ssl_eager_resume_continues_bit_for_bit(cfg, batches, tmp_dir):
    from regda_amd.checkpoint import load_training_state
    A = uninterrupted(cfg, batches, tmp_dir)
    c = ssl_step(cfg, init_seed=99, torch_seed=5, proto_seed=6)
    assert not torch.equal(c.model.flat_p, A['steps'][1]['p']) and c.first
    assert load_training_state(A['path'], c) == 2
    assert c.first is False
    steps = ssl_steps(c, cfg, batches, (2, 3))
    assert_same(A['steps'][2:], A['final'], steps, ssl_final(c), f'{cfg}: resumed')
    # control, the reference's practice: continue from the saved MODEL alone.  It must not reproduce the uninterrupted
    # run -- otherwise this test could not see a momentum (teacher, statistics, generator) that was never restored
    d = ssl_step(cfg, init_seed=99, torch_seed=5, proto_seed=6)
    d.model.load_state_dict(torch.load(A['path'], weights_only=True)['step']['model'], strict=True)
    assert torch.equal(d.model.flat_p, A['steps'][1]['p'])
    third = ssl_steps(d, cfg, batches, (2,))
    assert not torch.equal(third[0]['p'], A['steps'][2]['p'])


@pytest.mark.parametrize('cfg', ['online', 'offline'])
def test_ssl_resume_then_record_a_plan_without_an_eager_step(cfg, batches, tmp_dir):
    """record_plan() straight after the load (`first` is what was saved), step 3 is the recording, step 4 a replay"""
    from regda_amd.checkpoint import load_training_state
    A = uninterrupted(cfg, batches, tmp_dir)
    c = ssl_step(cfg, init_seed=99, torch_seed=5, proto_seed=6)
    load_training_state(A['path'], c)
    steps = ssl_steps(c, cfg, batches, (2, 3), record_at=2)
    assert c._plan is not None
    assert_same(A['steps'][2:], A['final'], steps, ssl_final(c), f'{cfg}: resumed into a new plan')


@pytest.mark.parametrize('cfg', ['online', 'offline'])
def test_ssl_resume_into_a_step_that_already_holds_a_plan(cfg, batches, tmp_dir):
    """The in-place rule: the plan was recorded on another trajectory (other weights, prototypes, seeds, batch order) and
    holds the addresses of the step's buffers; the load writes into those buffers, and the replays continue run A."""
    from regda_amd.checkpoint import load_training_state
    A = uninterrupted(cfg, batches, tmp_dir)
    c = ssl_step(cfg, init_seed=99, torch_seed=5, proto_seed=6)
    ssl_steps(c, cfg, batches, (3, 1), record_at=1)
    held = {k: getattr(c, k).data_ptr() for k in ('mom', 'prototypes')}
    held.update(p=c.model.flat_p.data_ptr(), pb=c.model.flat_pb.data_ptr(), buf=c.model.flat_buf.data_ptr())
    if cfg == 'offline':
        held.update(acc=c.loss_fn_t.acc_sum.data_ptr(), bw=c.loss_fn_t.bins_weight.data_ptr())
    else:
        held.update(shadow=c.teacher.flat_p.data_ptr(), shadow_b=c.teacher.flat_pb.data_ptr())
    plan = c._plan
    load_training_state(A['path'], c)
    now = {k: getattr(c, k).data_ptr() for k in ('mom', 'prototypes')}
    now.update(p=c.model.flat_p.data_ptr(), pb=c.model.flat_pb.data_ptr(), buf=c.model.flat_buf.data_ptr())
    if cfg == 'offline':
        now.update(acc=c.loss_fn_t.acc_sum.data_ptr(), bw=c.loss_fn_t.bins_weight.data_ptr())
    else:
        now.update(shadow=c.teacher.flat_p.data_ptr(), shadow_b=c.teacher.flat_pb.data_ptr())
    assert now == held and c._plan is plan
    steps = ssl_steps(c, cfg, batches, (2, 3))
    assert_same(A['steps'][2:], A['final'], steps, ssl_final(c), f'{cfg}: resumed into an existing plan')


def test_refused_states_name_the_entry_and_leave_the_step_as_it_was(batches, tmp_dir):
    """Every refusal is raised before anything is written: after all of them the step continues run A bit for bit."""
    from regda_amd.ssl import SSLStep
    A = uninterrupted('online', batches, tmp_dir)
    # the states to offer come first: building a model or a step draws from the generators the victim's steps draw from
    other = ssl_step('online', init_seed=99, torch_seed=5, proto_seed=6).state_dict()     # loadable, another trajectory
    seven = SSLStep(build(C=7), protos(1, C=7), class_num=7, ema_decay=0.9).state_dict()
    aspp = SSLStep(build(use_ppm=False), protos(1), ema_decay=0.9).state_dict()
    w, w_twin = ssl_step('plain'), ssl_step('plain')
    no_teacher = w.state_dict()
    v = ssl_step('online')
    ssl_steps(v, 'online', batches, range(2))
    own = v.state_dict()
    assert 'teacher' not in no_teacher and 'teacher' in own

    def refused(sd, match, exc=ValueError, strict=True):
        with pytest.raises(exc, match=match):
            v.load_state_dict(sd, strict=strict)

    refused(seven, 'class_num')
    refused(aspp, 'head_kind')
    refused(no_teacher, 'teacher')
    refused({k: x for k, x in other.items() if k != 'teacher'}, 'teacher')
    refused({k: x for k, x in other.items() if k != 'mom'}, 'mom')
    key = 'layer5.conv_last.4.weight'
    refused(dict(other, model={k: x for k, x in other['model'].items() if k != key}), key)
    refused(dict(other, format=99), 'format')
    refused({k: x for k, x in other.items() if k != 'format'}, 'format')
    refused(dict(other, kind='AlignStep'), 'kind')
    refused(dict(other, config=dict(other['config'], loss_t='gdp')), 'loss_t')
    # good up to its last entries: a load that wrote as it went would have replaced the weights by now
    refused(dict(other, prototypes=torch.zeros(6, 100)), 'prototypes')
    refused(dict(other, mom=other['mom'][:-64]), 'mom')
    refused(dict(other, rng=dict(cpu=other['rng']['cpu'])), 'cuda')
    refused(dict(other, prototypes=torch.zeros(6, 100)), 'prototypes', strict=False)
    v._graph = object()         # what capture() leaves; nothing of it is touched before the refusal
    refused(other, 'capture', exc=RuntimeError)
    v._graph = None
    steps = ssl_steps(v, 'online', batches, (2, 3))
    assert_same(A['steps'][2:], A['final'], steps, ssl_final(v), 'after the refusals')
    # the reverse: a step without a teacher that was offered one equals its twin that never was
    with pytest.raises(ValueError, match='teacher'):
        w.load_state_dict(own)
    torch.manual_seed(3)
    s1 = ssl_steps(w, 'plain', batches, (0,))
    torch.manual_seed(3)
    s2 = ssl_steps(w_twin, 'plain', batches, (0,))
    assert_same(s1, ssl_final(w), s2, ssl_final(w_twin), 'step without a teacher, after the refusal')


def test_the_file_is_plain_data(batches, tmp_dir):
    A = uninterrupted('offline', batches, tmp_dir)
    uninterrupted('online', batches, tmp_dir)
    for cfg in ('offline', 'online'):
        raw = torch.load(_CACHE[cfg]['path'], weights_only=True)
        assert sorted(raw) == ['format', 'iteration', 'step'] and raw['iteration'] == 2
        leaves = []

        def walk(x, where):
            if isinstance(x, dict):
                assert type(x) is dict and all(isinstance(k, str) for k in x), where
                for k, v in x.items():
                    walk(v, f'{where}.{k}')
            elif isinstance(x, list):
                for i, v in enumerate(x):
                    walk(v, f'{where}[{i}]')
            else:
                assert x is None or isinstance(x, (torch.Tensor, bool, int, float, str)), (where, type(x))
                assert not isinstance(x, torch.Tensor) or x.device.type == 'cpu', where
                leaves.append(where)
        walk(raw, 'file')
        sd = raw['step']
        assert sd['kind'] == 'SSLStep' and sd['first'] is False and len(sd['model']) == len(build().state_dict())
        assert sd['config']['model'] == dict(resnet_type=RT, head_kind='ppm', num_classes=6, n_param=sd['mom'].numel())
        assert ('teacher' in sd) == (cfg == 'online') and set(sd['rng']) == {'cpu', 'cuda'}
        if cfg == 'offline':
            assert set(sd['loss_fn_t']) == {'_extra_state'} and set(sd['loss_fn_t']['_extra_state']) == {'acc_sum', 'bins_weight'}
            assert set(sd['class_balancer_s']) == {'_extra_state'} and sd['class_balancer_t']['_extra_state']['freq'].shape == (6,)
            assert 'class_balancer._extra_state' in sd['loss_fn_s']
    assert 'rng' not in ssl_step('plain').state_dict(rng=False)
    assert A['final']['acc_sum'].abs().sum().item() > 0


# ------------------------------------------------------------------------------------------------------- stage 1 and 2
def align_step(init_seed=12, torch_seed=77, proto_seed=5):
    from regda_amd.align import AlignStep
    from regda_amd.models.Discriminator import FCDiscriminator
    m = build()
    m.load_state_dict(init_sd(init_seed), strict=True)
    torch.manual_seed(torch_seed)            # the discriminators' initialisation, then the Dropout2d seeds and the draws
    ds = [FCDiscriminator(6, ndf=32).cuda() for _ in range(2)]
    st = AlignStep(m, protos(proto_seed), adv_weight=0.5, contrast_weight=1e-2, discriminators=ds)
    st.contrast['max_views'] = 2             # low enough that classes of both domains qualify (asserted at every step)
    return st


def align_steps(st, batches, which):
    out = []
    for i in which:
        b = batches[i]
        r = st.step(b['images_s'], b['label_s'], b['images_t'], b['regs_t'], LRS[i])
        assert st.last_contrast[0] is not None and st.last_contrast[1] is not None, 'no draw was exercised'
        out.append(dict(loss_seg=r[0].clone(), loss_align=r[1].clone(), gn=r[2].clone(), loss_adv=st.loss_adv.clone(),
                        loss_disc=st.loss_disc.clone(), loss_contrast=st.loss_contrast.clone(), hard=st.last_hard.clone()))
    torch.cuda.synchronize()
    return out


def align_final(st):
    torch.cuda.synchronize()
    f = dict(p=st.model.flat_p.clone(), buf=st.model.flat_buf.clone(), mom=st.mom.clone(), protos=st.prototypes.clone())
    aligner = st.adv['aligner']
    for i, d in enumerate(aligner.discriminators):
        for k, p in d.named_parameters():
            f[f'disc{i}.{k}'] = p.detach().clone()
    for i, s in enumerate(aligner.optimizer.state_dict()['state'].values()):
        f[f'adam{i}.m'], f[f'adam{i}.v'] = s['exp_avg'].clone(), s['exp_avg_sq'].clone()
    return f


def test_align_step_with_adversarial_and_contrast_terms_resumes_bit_for_bit(batches, tmp_path):
    from regda_amd.checkpoint import load_training_state, save_training_state
    a = align_step()
    A = align_steps(a, batches, range(4))
    assert all(s[k].item() != 0.0 for s in A for k in ('loss_adv', 'loss_disc', 'loss_contrast'))
    b = align_step()
    align_steps(b, batches, range(2))
    path = os.path.join(tmp_path, 'align.pth')
    save_training_state(path, b, 2)
    c = align_step(init_seed=99, torch_seed=5, proto_seed=6)
    assert not torch.equal(c.adv['aligner'].discriminators[0].conv1.weight, b.adv['aligner'].discriminators[0].conv1.weight)
    assert load_training_state(path, c) == 2
    steps = align_steps(c, batches, (2, 3))
    assert_same(A[2:], align_final(a), steps, align_final(c), 'stage 2: resumed')
    # a state without the aligner's entry, and one for other discriminators, are refused by name
    sd = torch.load(path, weights_only=True)['step']
    assert sd['kind'] == 'AlignStep' and len(sd['adv']['discriminators']) == 2
    with pytest.raises(ValueError, match='adv'):
        c.load_state_dict({k: v for k, v in sd.items() if k != 'adv'})
    with pytest.raises(ValueError, match='discriminators'):
        c.load_state_dict(dict(sd, adv=dict(sd['adv'], discriminators=sd['adv']['discriminators'][:1])))
    assert_same([], align_final(a), [], align_final(c), 'stage 2: after the refusals')


def source_step(init_seed=12, torch_seed=77):
    from regda_amd.gast.balance import ClassBalance
    from regda_amd.source import SourceStep
    m = build()
    m.load_state_dict(init_sd(init_seed), strict=True)
    torch.manual_seed(torch_seed)
    return SourceStep(m, class_balancer_s=ClassBalance(class_num=6, ignore_label=-1, decay=0.99, temperature=0.5),
                      align_domain=True)


def source_steps(st, batches, which):
    out = []
    for i in which:
        b = batches[i]
        r = st.step(b['images_s'], b['label_s'], b['images_t'], LRS[i])
        out.append(dict(loss_seg=r[0].clone(), loss_domain=r[1].clone(), gn=r[2].clone()))
    torch.cuda.synchronize()
    return out


def source_final(st):
    return dict(p=st.model.flat_p.clone(), buf=st.model.flat_buf.clone(), mom=st.mom.clone(),
                freq=st.class_balancer_s.freq.clone())


def test_source_step_with_domain_alignment_resumes_bit_for_bit(batches, tmp_path):
    from regda_amd.checkpoint import load_training_state, save_training_state
    a = source_step()
    A = source_steps(a, batches, range(3))
    assert all(s['loss_domain'].item() != 0.0 for s in A)
    b = source_step()
    source_steps(b, batches, range(1))
    path = os.path.join(tmp_path, 'source.pth')
    save_training_state(path, b, 1)
    c = source_step(init_seed=99, torch_seed=5)
    assert load_training_state(path, c) == 1
    assert_same(A[1:], source_final(a), source_steps(c, batches, (1, 2)), source_final(c), 'stage 1: resumed')
    with pytest.raises(ValueError, match='kind'):
        ssl_step('plain').load_state_dict(torch.load(path, weights_only=True)['step'])


# ------------------------------------------------------- format-1 states written while both steps derived from SSLStep
def test_a_source_step_has_no_prototypes_and_loads_a_state_that_carries_them(batches):
    """Such a state holds the zero tensor that stood in for prototypes and the SSL step's two config keys: it loads under
    strict=True, the entries are ignored, and the run continues with the bits of one that loaded today's form."""
    a = source_step()
    assert not hasattr(a, 'prototypes') and not hasattr(a, 'loss_fn_t') and a.teacher is None
    source_steps(a, batches, range(1))
    sd = a.state_dict()
    assert 'prototypes' not in sd and 'loss_t' not in sd['config'] and 'ema_decay' not in sd['config']
    old = dict(sd, prototypes=torch.zeros(6, 2048), config=dict(sd['config'], loss_t='none', ema_decay=None))
    b, c = source_step(init_seed=99, torch_seed=5), source_step(init_seed=99, torch_seed=6)
    b.load_state_dict(sd, strict=True)          # (the generators a state restores are global: load, then run, one by one)
    new_form = source_steps(b, batches, (1, 2))
    with pytest.raises(ValueError, match='no_such_entry'):
        c.load_state_dict(dict(old, no_such_entry=torch.zeros(1)), strict=True)
    c.load_state_dict(old, strict=True)
    assert not hasattr(c, 'prototypes') and 'prototypes' not in c.state_dict()
    assert_same(new_form, source_final(b), source_steps(c, batches, (1, 2)), source_final(c),
                'stage 1: the earlier form of the state')


def test_an_align_step_loads_a_state_that_carries_the_ssl_config_keys(batches):
    a = align_step()
    assert not hasattr(a, 'loss_fn_t') and a.teacher is None
    align_steps(a, batches, range(1))
    sd = a.state_dict()
    assert 'loss_t' not in sd['config'] and 'ema_decay' not in sd['config'] and 'prototypes' in sd
    # built on a second copy of the state: a load may keep what it is given (torch's Adam keeps the CPU `step` tensors)
    old = a.state_dict()
    old = dict(old, config=dict(old['config'], loss_t='none', ema_decay=None))
    b, c = align_step(init_seed=99, torch_seed=5, proto_seed=6), align_step(init_seed=99, torch_seed=6, proto_seed=7)
    b.load_state_dict(sd, strict=True)
    new_form = align_steps(b, batches, (1, 2))
    with pytest.raises(ValueError, match='no_such_entry'):
        c.load_state_dict(dict(old, no_such_entry=torch.zeros(1)), strict=True)
    c.load_state_dict(old, strict=True)
    assert_same(new_form, align_final(b), align_steps(c, batches, (1, 2)), align_final(c),
                'stage 2: the earlier form of the state')


# ------------------------------------------------------------------------------------------ the helpers a script holds
def test_aligner_and_loss_modules_round_trip(gold):
    """Aligner (prototypes and the update_avg totals, before and after the first batch), GHMLoss and GDPLoss with its own
    balancer through the standard nn.Module methods: loaded in place, and the next update continues bit for bit."""
    import numpy as np
    from regda_amd.gast.alignment import Aligner
    from regda_amd.gast.balance import GDPLoss, GHMLoss
    g = gold('proto_init.npz')
    batch = lambda i: (torch.from_numpy(g[f'feat{i}']).cuda(), torch.from_numpy(g[f'lab{i}'].astype(np.int64)).cuda())
    a, b = (Aligner(None, feat_channels=64, class_num=6, ignore_label=-1) for _ in range(2))
    empty = a.state_dict()
    assert empty['data_sum'] is None and empty['data_cnt'] is None
    a.update_avg(*batch(0))
    a.init_avg()
    a.update_prototype(*batch(1))
    sd = a.state_dict()
    assert sd['data_sum'].shape == (6, 64) and sd['data_cnt'].shape == (6, 1) and sd['prototypes'].device.type == 'cpu'
    held = b.prototypes
    b.load_state_dict(sd)
    assert b.prototypes is held and torch.equal(b.prototypes, a.prototypes)
    for x in (a, b):
        x.update_avg(*batch(2))
        x.update_prototype(*batch(2))
    assert torch.equal(a.data_sum, b.data_sum) and torch.equal(a.data_cnt, b.data_cnt)
    assert torch.equal(a.prototypes, b.prototypes) and a.data_cnt.sum().item() > 0
    before = b.state_dict()
    with pytest.raises(ValueError, match='prototypes'):
        b.load_state_dict(dict(sd, prototypes=torch.zeros(7, 64)))
    with pytest.raises(ValueError, match='data_cnt'):
        b.load_state_dict({k: v for k, v in sd.items() if k != 'data_cnt'})
    with pytest.raises(ValueError, match='data_sum'):
        Aligner(None, feat_channels=32, class_num=6).load_state_dict(dict(sd, prototypes=torch.zeros(6, 32)))
    assert all(torch.equal(before[k], v) for k, v in b.state_dict().items())
    b.load_state_dict(empty)
    assert b._avg_stats is None and b.prototypes is held and b.prototypes.abs().max().item() == 0.0
    # the loss modules: statistics as extra state of the standard state_dict()
    logits = [torch.randn(2, 6, 8, 8, generator=torch.Generator().manual_seed(i)).cuda() for i in range(2)]
    labels = torch.randint(-1, 6, (2, 128, 128), generator=torch.Generator().manual_seed(2)).cuda()
    for make in (lambda: GHMLoss(bins=30, momentum=0.9, ignore_label=-1),
                 lambda: GDPLoss(bins=30, momentum=0.9, class_num=6, ignore_label=-1, class_balance=True)):
        p, q = make(), make()
        p(logits[0], labels)
        sd = {k: (v if torch.is_tensor(v) else {n: t.clone() for n, t in v.items()}) for k, v in p.state_dict().items()}
        held = q.acc_sum
        q.load_state_dict(sd)
        assert q.acc_sum is held and torch.equal(q.acc_sum, p.acc_sum) and q.acc_sum.abs().sum().item() > 0
        if p.kind == 'gdp':
            assert set(sd) == {'_extra_state', 'class_balancer._extra_state'}
            assert torch.equal(q.class_balancer.freq, p.class_balancer.freq) and torch.equal(q.bins_weight, p.bins_weight)
        assert torch.equal(p(logits[1], labels), q(logits[1], labels)) and torch.equal(q.acc_sum, p.acc_sum)
        with pytest.raises(ValueError, match='acc_sum'):
            q.load_state_dict(dict(sd, _extra_state=dict(sd['_extra_state'], acc_sum=torch.zeros(10))))
