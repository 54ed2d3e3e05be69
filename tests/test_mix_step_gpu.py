"""GPU: DACS inside the SSL step (SSLStep(mix=DomainMix)): the teacher labels the clean tile, the student sees the mixed
one, and the source labels are pasted onto the pseudo labels after selection and LRH.  Steps are bit-reproducible
(tests/test_determinism_gpu.py) and the mixing kernels copy, so every comparison is torch.equal.

Shapes: the shallow resnet17t topology, 2 + 2 tiles of 64 x 64 or 128 x 128 from make_batch, fixed drop masks."""
import numpy as np
import pytest
import torch

import mix_select_ref
from oracle import model as omodel

pytestmark = pytest.mark.gpu

RT = 'resnet17t'
C = 6


def build():
    from regda_amd.models.Encoder import Deeplabv2
    return Deeplabv2(dict(backbone=dict(resnet_type=RT, output_stride=16, pretrained=False), multi_layer=True,
                          cascade=False, use_ppm=True, ppm=dict(num_classes=C, use_aux=False, fc_dim=2048),
                          inchannels=2048, num_classes=C, is_ins_norm=True))


_INIT = {}


def init_sd(seed=12):
    """the oracle's initial weights of a seed: made once, shared, never written"""
    if seed not in _INIT:
        _INIT[seed] = omodel.init_state_dict(RT, C, seed=seed)
    return _INIT[seed]


_BATCH = {}


def batch(size, seed):
    from regda_amd.synthetic import make_batch
    if (size, seed) not in _BATCH:
        _BATCH[size, seed] = make_batch(b=2, size=size, seed=seed)
    return _BATCH[size, seed]


def new_step(mix=None, init_seed=12, proto_seed=5, **kw):
    from regda_amd.ssl import SSLStep
    m = build()
    m.load_state_dict(init_sd(init_seed), strict=True)
    m.set_drop_masks(torch.ones(4, 512), torch.ones(4, 512))
    protos = torch.randn(C, 2048, generator=torch.Generator().manual_seed(proto_seed))
    return SSLStep(m, protos, mix=mix, **kw)


def class_mask(st, label_s):
    """the pasted pixels of the step's last draw, from the table its kernels read (class mode)"""
    bits = st.last_mix_table[:, 0].to(torch.int64).view(-1, 1, 1) & 0xFFFFFFFF
    lab = label_s.reshape(label_s.shape[0], label_s.shape[-2], label_s.shape[-1])
    return (lab >= 0) & (lab < C) & (((bits >> lab.clamp(0, 31)) & 1) == 1)


def regs_of(b):
    return b['regs_t'].squeeze(1).contiguous()


def test_teacher_sees_the_clean_tile_and_the_callers_tile_is_not_written():
    from regda_amd.aug.mix import DomainMix
    b = batch(64, 3)
    st = new_step(DomainMix('class', C, seed=2), ema_decay=0.9)
    before = st.teacher_probs(b['images_t']).clone()
    img_t, img_s, lab_s = b['images_t'].clone(), b['images_s'].clone(), b['label_s'].clone()
    st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 0.0)
    torch.cuda.synchronize()
    assert st.last_mix is not None and st.last_mix[0] == 'classes' and len(st.last_mix[1]) == 3
    mask = class_mask(st, b['label_s'])
    assert mask.any() and not mask.all()
    assert torch.equal(st.last_soft_t, before)          # the teacher's view of the CLEAN tile
    assert torch.equal(b['images_t'], img_t) and torch.equal(b['images_s'], img_s) and torch.equal(b['label_s'], lab_s)
    assert st.mix_flag_value() == 0


def test_labels_without_refinement_are_the_clean_tiles_outside_the_mask_and_the_sources_on_it():
    from regda_amd import ops
    from regda_amd.aug.mix import DomainMix
    b = batch(64, 3)
    st = new_step(DomainMix('class', C, seed=2), ema_decay=0.9, refine_label=False)
    st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 0.0)
    torch.cuda.synchronize()
    soft = st.last_soft_t
    clean = ops.lrh(ops.pseudo_select(soft, st.top, st.low, -1), regs_of(b), st.percent, C, -1, st.max_regions)
    mask = class_mask(st, b['label_s'])
    assert mask.any() and not mask.all()
    assert torch.equal(st.last_hard, torch.where(mask, b['label_s'], clean))
    assert not torch.equal(st.last_hard, clean)


@pytest.mark.parametrize('kind', ['class', 'box'])
def test_labels_with_refinement_match_a_plain_step_on_the_premixed_tile(kind):
    """The mixed step against a step without a mix that is GIVEN the mixed tile and the teacher's clean soft labels:
    the same student forward, so the same source loss, and the same pseudo labels away from the paste -- with the fused
    pseudo_lrh route (keep_debug off) and the two-call route (on)."""
    from regda_amd import ops
    from regda_amd.aug.mix import DomainMix
    b = batch(64, 21)
    runs = {}
    for debug in (False, True):
        st = new_step(DomainMix(kind, C, seed=7), ema_decay=0.9)
        st.keep_debug = debug
        ls, lt, _ = st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)
        torch.cuda.synchronize()
        runs[debug] = (st, ls.clone(), lt.clone(), st.last_hard.clone())
    st = runs[False][0]
    mode = ops.MIX_BOX if kind == 'box' else ops.MIX_CLASS
    mixed = ops.domain_mix_table(b['images_s'], b['label_s'], st.last_mix_table, mode, images_in=b['images_t'],
                                 images_out=torch.empty_like(b['images_t']), class_num=C)[0]
    assert not torch.equal(mixed, b['images_t'])
    if kind == 'class':
        mask = class_mask(st, b['label_s'])
    else:
        y0, y1, x0, x1 = st.last_mix[1]
        assert st.last_mix_table.cpu().tolist() == [[0, y0, y1, x0, x1, 0, 0, 0]] * 2
        mask = torch.zeros_like(b['label_s'], dtype=torch.bool)
        mask[:, y0:y1, x0:x1] = True
    assert mask.any() and not mask.all()
    plain = new_step(None)
    ls, lt, _ = plain.step(b['images_s'], b['label_s'], mixed, st.last_soft_t.clone(), b['regs_t'], 1e-3)
    torch.cuda.synchronize()
    want = torch.where(mask, b['label_s'], plain.last_hard)
    for debug in (False, True):
        assert torch.equal(runs[debug][1], ls), 'source loss'
        assert torch.equal(runs[debug][3], want), 'last_hard, keep_debug=%s' % debug
    assert not torch.equal(want, plain.last_hard)


@pytest.mark.parametrize('loss_t,refine', [('none', False), ('uvem', False), ('uvem', True), ('gdp', False)])
def test_target_loss_reads_the_pasted_labels(loss_t, refine):
    from regda_amd import ops
    from regda_amd.aug.mix import DomainMix
    from regda_amd.gast.balance import target_loss
    b = batch(64, 22)
    st = new_step(DomainMix('class', C, seed=3), refine_label=refine, loss_t=loss_t)
    st.keep_debug = True
    protos_before = st.prototypes.clone()
    soft_in = b['soft_t'].clone()
    _, lt, _ = st.step(b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'], 1e-3)
    torch.cuda.synchronize()
    assert torch.equal(b['soft_t'], soft_in), "the caller's soft labels were written"
    d = st.debug
    ids = st.last_mix[1]
    mask = class_mask(st, b['label_s'])
    assert mask.any() and not mask.all()
    hard = torch.where(mask, b['label_s'], d['hard_clean'])
    assert torch.equal(st.last_hard, hard)
    soft = d['soft'].clone()            # the refined soft label (the input itself without refinement), then the one-hot
    assert torch.equal(soft, soft_in) or refine
    ops.domain_mix(b['images_s'], b['label_s'], b['images_t'].clone(), soft_t=soft, classes=ids, class_num=C)
    fresh = target_loss(loss_t, None, 0.2, 0.7, 4.0, C, -1, device='cuda', gdp_prototype=True)      # statistics as the step's stood before
    g1, g2 = torch.empty_like(d['g1_t']), torch.empty_like(d['g2_t'])
    kw = {}
    if loss_t == 'gdp':
        kw['pixel_weight'] = ops.proto_pixel_weight(d['feat_t'], protos_before, hard, ignore_label=-1)
        assert torch.equal(kw['pixel_weight'], st.last_proto_weight)
    want = fresh.launch(d['t1'], d['t2'], hard, soft=soft if loss_t == 'uvem' else None, g1=g1, g2=g2, **kw)[0]
    torch.cuda.synchronize()
    assert torch.equal(lt.reshape(-1), want.reshape(-1)), 'target loss'
    assert torch.equal(d['g1_t'], g1) and torch.equal(d['g2_t'], g2), 'target logit gradients'
    if loss_t == 'uvem':
        assert torch.equal(d['soft_loss'], soft) and not torch.equal(soft, d['soft'])


def test_dacs_table_is_the_numpy_rule_on_the_source_labels_and_the_drawn_ranks():
    from regda_amd.aug.mix import DomainMix
    b = batch(64, 22)
    st = new_step(DomainMix('dacs', C, seed=9), ema_decay=0.9)
    twin = DomainMix('dacs', C, seed=9)
    for i in range(2):
        st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)
        torch.cuda.synchronize()
        kind, ranks = st.last_mix
        assert kind == 'ranks' and np.array_equal(ranks, twin.draw_step(2, 64, 64)[1])
        table = st.last_mix_table.cpu().numpy()
        bits, flag = mix_select_ref.select_classes(b['label_s'].cpu().numpy(), ranks)
        assert table[:, 0].view(np.uint32).tolist() == bits.tolist() and (table[:, 1:] == 0).all()
        assert flag == 0 and st.mix_flag_value() == 0
        mask = class_mask(st, b['label_s'])
        assert mask.any() and not mask.all()
        assert torch.equal(st.last_hard[mask], b['label_s'][mask])


@pytest.mark.parametrize('kind', ['class', 'dacs'])
def test_a_batch_that_is_not_mixed_equals_the_step_without_a_mix(kind):
    from regda_amd.aug.mix import DomainMix
    b = batch(64, 22)
    outs = []
    for mix in (DomainMix(kind, C, prob=0.0, seed=1), None):
        st = new_step(mix, loss_t='uvem')
        ls, lt, gn = st.step(b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'], 1e-3)
        torch.cuda.synchronize()
        outs.append((ls.clone(), lt.clone(), gn.clone(), st.last_hard.clone(), st.model.flat_p.clone()))
        if mix is not None:
            assert st.last_mix is None and (st.last_mix_table.cpu().numpy() == 0).all()
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_plan_replay_matches_the_eager_steps_and_capture_refuses():
    """One eager step, record_plan on the second, three replays, against five eager steps: the draw and the table write
    are a host action of the plan, the select and the two table launches rows of its table."""
    from regda_amd.aug.mix import DomainMix
    seq = [batch(128, 21), batch(128, 21), batch(128, 22), batch(128, 21), batch(128, 22)]
    lrs = [1e-3, 1e-3, 1e-3, 3e-3, 1e-3]

    def run(use_plan):
        st = new_step(DomainMix('dacs', C, seed=13), ema_decay=0.9)
        out = []
        for i, (b, lr) in enumerate(zip(seq, lrs)):
            args = (b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'])
            if use_plan and i == 1:
                st.record_plan(*args, lr=lr)
                o = st._out
            else:
                o = st.step(*args, lr)
            torch.cuda.synchronize()
            out.append(dict(ls=o[0].clone(), lt=o[1].clone(), gn=o[2].clone(), hard=st.last_hard.clone(),
                            table=st.last_mix_table.clone(), ranks=torch.from_numpy(st.last_mix[1].copy())))
        return st, out

    st_e, out_e = run(False)
    st_p, out_p = run(True)
    assert st_p._plan is not None and st_e._plan is None
    for i, (x, y) in enumerate(zip(out_e, out_p)):
        for k in x:
            assert torch.equal(x[k], y[k]), 'step %d: %s differs' % (i, k)
    for a, bb in zip(out_p, out_p[1:]):
        assert not torch.equal(a['ranks'], bb['ranks'])         # a replay re-runs the draw
    assert len({tuple(o['table'][:, 0].tolist()) for o in out_p}) > 1
    assert torch.equal(st_p.model.flat_p, st_e.model.flat_p) and torch.equal(st_p.model.flat_buf, st_e.model.flat_buf)
    assert torch.equal(st_p.teacher.flat_p, st_e.teacher.flat_p) and torch.equal(st_p.prototypes, st_e.prototypes)
    b = seq[0]
    with pytest.raises(RuntimeError, match='record_plan'):
        st_e.capture(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'])


def test_plan_replay_pastes_into_a_fresh_copy_of_the_soft_labels():
    """refine_label=False with a target loss that reads the soft label: the copy the one-hot is pasted into is made at
    every replay, from that replay's soft labels, and the caller's tensor stays as it was."""
    from regda_amd.aug.mix import DomainMix
    seq = [batch(64, 21), batch(64, 21), batch(64, 22), batch(64, 21)]

    def run(use_plan):
        st = new_step(DomainMix('class', C, seed=4), refine_label=False, loss_t='uvem')
        out = []
        for i, b in enumerate(seq):
            args = (b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'])
            keep = b['soft_t'].clone()
            if use_plan and i == 1:
                st.record_plan(*args, lr=1e-3)
                o = st._out
            else:
                o = st.step(*args, 1e-3)
            torch.cuda.synchronize()
            assert torch.equal(b['soft_t'], keep)
            out.append((o[0].clone(), o[1].clone(), st.last_hard.clone()))
        return st, out

    st_e, out_e = run(False)
    st_p, out_p = run(True)
    for i, (x, y) in enumerate(zip(out_e, out_p)):
        assert all(torch.equal(a, b) for a, b in zip(x, y)), 'step %d' % i
    assert torch.equal(st_p.model.flat_p, st_e.model.flat_p)


def test_resume_continues_the_draws(tmp_path):
    from regda_amd.aug.mix import DomainMix
    from regda_amd.checkpoint import load_training_state, save_training_state
    seq = [batch(64, 21), batch(64, 22), batch(64, 21)]

    def steps(st, which):
        draws = []
        for i in which:
            b = seq[i]
            st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)
            draws.append(st.last_mix[1].copy())
        torch.cuda.synchronize()
        return draws

    a = new_step(DomainMix('dacs', C, seed=31), ema_decay=0.9)
    torch.manual_seed(77)
    draws_a = steps(a, range(3))
    b = new_step(DomainMix('dacs', C, seed=31), ema_decay=0.9)
    torch.manual_seed(77)
    steps(b, range(1))
    path = str(tmp_path / 'mix.pth')
    save_training_state(path, b, 1)
    c = new_step(DomainMix('dacs', C, seed=99), init_seed=13, proto_seed=6, ema_decay=0.9)      # other seeds throughout
    torch.manual_seed(5)
    assert load_training_state(path, c) == 1
    draws_c = steps(c, range(1, 3))
    assert all(np.array_equal(x, y) for x, y in zip(draws_a[1:], draws_c))
    assert not np.array_equal(draws_a[1], draws_a[2])
    assert torch.equal(c.model.flat_p, a.model.flat_p) and torch.equal(c.teacher.flat_p, a.teacher.flat_p)
    assert torch.equal(c.mom, a.mom) and torch.equal(c.prototypes, a.prototypes)
    plain = new_step(None, ema_decay=0.9)
    with pytest.raises(ValueError, match='mix'):
        load_training_state(path, plain)


def test_the_other_steps_refuse_a_mix():
    from regda_amd.align import AlignStep
    from regda_amd.aug.mix import DomainMix
    from regda_amd.source import SourceStep
    mx = DomainMix('class', C, seed=1)
    with pytest.raises(NotImplementedError, match='SSL step'):
        AlignStep(None, None, mix=mx)
    with pytest.raises(NotImplementedError, match='SSL step'):
        SourceStep(None, mix=mx)
