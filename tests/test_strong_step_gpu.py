"""GPU: the strong augmentation inside the SSL step (SSLStep(strong=StrongAugment)): the student's target tile is
jittered and blurred after the mix, the teacher and the caller's tensors see nothing of it.  Steps are bit-reproducible
(tests/test_determinism_gpu.py) and the image mean of the contrast step is an integer sum, so every comparison is
torch.equal.

Shapes and helpers are those of tests/test_mix_step_gpu.py: the shallow resnet17t topology, 2 + 2 tiles of 64 x 64."""
import numpy as np
import pytest
import torch

from test_mix_step_gpu import C, batch, new_step

pytestmark = pytest.mark.gpu


def strong(seed, **kw):
    from regda_amd.aug.strong import StrongAugment
    kw.setdefault('jitter_prob', 0.7)
    kw.setdefault('blur_prob', 0.7)
    return StrongAugment(seed=seed, **kw)


def dacs(seed):
    from regda_amd.aug.mix import DomainMix
    return DomainMix('dacs', C, seed=seed)


def args_of(b, soft=False):
    return b['images_s'], b['label_s'], b['images_t'], b['soft_t'] if soft else None, b['regs_t']


def test_student_sees_the_augmented_mixed_tile_and_the_teacher_the_clean_one():
    from regda_amd import ops
    b = batch(64, 3)
    keep = {k: b[k].clone() for k in ('images_t', 'images_s', 'label_s', 'regs_t')}
    sa = strong(4, jitter_prob=1.0, blur_prob=1.0)
    st = new_step(dacs(2), ema_decay=0.9, strong=sa)
    st.keep_debug = True
    ls, lt, _ = st.step(*args_of(b), 1e-3)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(b[k], v), k + ' was written'
    assert st.last_strong.shape == (2, 8) and (st.last_strong[:, 5] == 3).all()
    assert np.array_equal(st.last_strong, strong(4, jitter_prob=1.0, blur_prob=1.0).draw(2))
    plain = new_step(dacs(2), ema_decay=0.9)
    plain.keep_debug = True
    _, lt0, _ = plain.step(*args_of(b), 1e-3)
    torch.cuda.synchronize()
    assert torch.equal(st.last_soft_t, plain.last_soft_t), "the teacher's soft labels"
    assert torch.equal(st.last_mix_table, plain.last_mix_table)
    mixed = ops.domain_mix_table(b['images_s'], b['label_s'], st.last_mix_table, ops.MIX_CLASS, images_in=b['images_t'],
                                 images_out=torch.empty_like(b['images_t']), class_num=C)[0]
    assert torch.equal(plain.debug['student_t'], mixed) and not torch.equal(mixed, b['images_t'])
    table = ops.strong_write_table(torch.empty(2, 8, device='cuda'), st.last_strong, (64, 64))
    want = ops.strong_augment(mixed, table, sa.mean, sa.std)
    assert torch.equal(st.debug['student_t'], want) and (want - mixed).abs().max() > 0.05
    assert torch.isfinite(ls).all() and torch.isfinite(lt).all() and not torch.equal(lt, lt0)
    assert st.strong_flag_value() == 0 and st.mix_flag_value() == 0


def test_strong_without_a_mix_leaves_the_callers_tile_alone():
    from regda_amd import ops
    b = batch(64, 21)
    img_t, soft_t = b['images_t'].clone(), b['soft_t'].clone()
    sa = strong(6, jitter_prob=1.0, blur_prob=1.0)
    st = new_step(None, strong=sa, loss_t='uvem')
    st.keep_debug = True
    ls, lt, _ = st.step(*args_of(b, soft=True), 1e-3)
    torch.cuda.synchronize()
    assert torch.equal(b['images_t'], img_t) and torch.equal(b['soft_t'], soft_t)
    table = ops.strong_write_table(torch.empty(2, 8, device='cuda'), st.last_strong, (64, 64))
    assert torch.equal(st.debug['student_t'], ops.strong_augment(b['images_t'], table, sa.mean, sa.std))
    assert st.debug['student_t'].data_ptr() != b['images_t'].data_ptr()
    # both coins off: the copy, and so the step without the option
    off = new_step(None, strong=strong(6, jitter_prob=0.0, blur_prob=0.0), loss_t='uvem')
    plain = new_step(None, loss_t='uvem')
    outs = []
    for s in (off, plain):
        o = s.step(*args_of(b, soft=True), 1e-3)
        torch.cuda.synchronize()
        outs.append((o[0].clone(), o[1].clone(), o[2].clone(), s.last_hard.clone(), s.model.flat_p.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    assert not torch.equal(lt, outs[1][1])


def run_steps(seq, use_plan=False, st=None, which=None, seed=13):
    st = st if st is not None else new_step(dacs(seed), ema_decay=0.9, strong=strong(seed + 1))
    out = []
    for i in (which if which is not None else range(len(seq))):
        a = args_of(seq[i])
        if use_plan and i == 1:
            st.record_plan(*a, lr=1e-3)
            o = st._out
        else:
            o = st.step(*a, 1e-3)
        torch.cuda.synchronize()
        out.append(dict(ls=o[0].clone(), lt=o[1].clone(), gn=o[2].clone(), hard=st.last_hard.clone(),
                        mix=st.last_mix_table.clone(), strong=torch.from_numpy(st.last_strong.copy())))
    return st, out


def same_state(a, b):
    return (torch.equal(a.model.flat_p, b.model.flat_p) and torch.equal(a.model.flat_buf, b.model.flat_buf)
            and torch.equal(a.teacher.flat_p, b.teacher.flat_p) and torch.equal(a.mom, b.mom)
            and torch.equal(a.prototypes, b.prototypes))


def test_two_runs_of_a_seed_and_a_recorded_plan_give_the_same_bits_and_capture_refuses():
    """Eager twice, and one eager step + record_plan on the second + two replays: losses, masks, tables and weights bit
    for bit; the draw is a host action of the plan, so every replay draws afresh."""
    seq = [batch(64, 21), batch(64, 21), batch(64, 22), batch(64, 21)]
    st_a, out_a = run_steps(seq)
    st_b, out_b = run_steps(seq)
    st_p, out_p = run_steps(seq, use_plan=True)
    assert st_p._plan is not None and st_a._plan is None
    for name, other in (('second run', out_b), ('plan', out_p)):
        for i, (x, y) in enumerate(zip(out_a, other)):
            for k in x:
                assert torch.equal(x[k], y[k]), '%s, step %d: %s differs' % (name, i, k)
    assert same_state(st_a, st_b) and same_state(st_a, st_p)
    for x, y in zip(out_p, out_p[1:]):
        assert not torch.equal(x['strong'], y['strong'])        # a replay re-runs the draw
    assert len({tuple(o['strong'][:, 5].tolist()) for o in out_p}) > 1
    with pytest.raises(RuntimeError, match='record_plan'):
        st_a.capture(*args_of(seq[0]))
    only = new_step(None, ema_decay=0.9, strong=strong(1))
    only.step(*args_of(seq[0]), 1e-3)
    with pytest.raises(RuntimeError, match=r'strong=.*record_plan'):
        only.capture(*args_of(seq[0]))


def test_resume_after_step_two_of_four_continues_bit_for_bit(tmp_path):
    from regda_amd.checkpoint import load_training_state, save_training_state
    seq = [batch(64, 21), batch(64, 22), batch(64, 21), batch(64, 22)]
    torch.manual_seed(77)
    a, out_a = run_steps(seq, seed=31)
    torch.manual_seed(77)
    b, _ = run_steps(seq, which=range(2), seed=31)
    path = str(tmp_path / 'strong.pth')
    save_training_state(path, b, 2)
    c = new_step(dacs(99), init_seed=13, proto_seed=6, ema_decay=0.9, strong=strong(98))    # other seeds throughout
    torch.manual_seed(5)
    assert load_training_state(path, c) == 2
    _, out_c = run_steps(seq, st=c, which=range(2, 4))
    for i, (x, y) in enumerate(zip(out_a[2:], out_c)):
        for k in x:
            assert torch.equal(x[k], y[k]), 'step %d: %s differs' % (i + 2, k)
    assert same_state(a, c)
    assert not torch.equal(out_a[2]['strong'], out_a[3]['strong'])
    # a state with 'strong' and a step without one, and the other way round
    with pytest.raises(ValueError, match='strong'):
        load_training_state(path, new_step(dacs(1), ema_decay=0.9))
    without = str(tmp_path / 'plain.pth')
    save_training_state(without, new_step(dacs(1), ema_decay=0.9), 0)
    with pytest.raises(ValueError, match='strong'):
        load_training_state(without, new_step(dacs(1), ema_decay=0.9, strong=strong(2)))
    bad = b.state_dict()        # (the state after step 2; c stands after step 4)
    bad['strong'] = {'rng': dict(bad['strong']['rng'], bit_generator='MT19937')}
    with pytest.raises(ValueError, match='step.strong'):
        c.load_state_dict(bad)
    assert same_state(a, c)     # validated before anything is written
