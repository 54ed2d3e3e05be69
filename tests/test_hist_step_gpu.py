"""GPU: histogram matching inside the fused steps (style=HistogramStyle): the source tile is matched into a buffer of the
step's own ahead of the forward, the teacher and the caller's tensors see nothing of it.  Steps are bit-reproducible
(tests/test_determinism_gpu.py) and the transform sums integers only, so every comparison is torch.equal.

Shapes and helpers are those of tests/test_mix_step_gpu.py: the shallow resnet17t topology, 2 + 2 tiles of 64 x 64.  The
same steps with style=FourierStyle: tests/test_fourier_step_gpu.py."""
import numpy as np
import pytest
import torch

from test_mix_step_gpu import C, batch, build, init_sd, new_step

pytestmark = pytest.mark.gpu


def style(seed, **kw):
    from regda_amd.aug.histogram import HistogramStyle
    kw.setdefault('blend', (0.3, 1.0))
    kw.setdefault('prob', 0.7)
    return HistogramStyle(seed=seed, **kw)


def dacs(seed):
    from regda_amd.aug.mix import DomainMix
    return DomainMix('dacs', C, seed=seed)


def strong(seed):
    from regda_amd.aug.strong import StrongAugment
    return StrongAugment(seed=seed, jitter_prob=0.7, blur_prob=0.7)


def args_of(b, soft=False):
    return b['images_s'], b['label_s'], b['images_t'], b['soft_t'] if soft else None, b['regs_t']


def matched(b, hs, table):
    from regda_amd.aug import histogram
    td = histogram.hist_style_write_table(torch.empty(2, 4, dtype=torch.int32, device='cuda'), table, 2, (64, 64))
    return histogram.hist_style(b['images_s'], b['images_t'], td, hs.mean_s, hs.std_s, hs.mean_t, hs.std_t)


def test_style_alone_matches_the_source_tile_into_a_buffer_of_the_steps_own():
    b = batch(64, 3)
    keep = {k: b[k].clone() for k in ('images_t', 'images_s', 'label_s', 'regs_t', 'soft_t')}
    hs = style(4, prob=1.0)
    st = new_step(None, style=hs, loss_t='uvem')
    st.keep_debug = True
    ls, lt, _ = st.step(*args_of(b, soft=True), 1e-3)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(b[k], v), k + ' was written'
    assert st.last_style.shape == (2, 4) and st.last_style.dtype == np.int32 and (st.last_style[:, 2] == 1).all()
    assert np.array_equal(st.last_style, style(4, prob=1.0).draw(2, 2, 64, 64))
    want = matched(b, hs, st.last_style)
    assert torch.equal(st.debug['source_s'], want) and (want - b['images_s']).abs().max() > 1.0 / 64     # a grey level
    assert st.debug['source_s'].data_ptr() != b['images_s'].data_ptr()
    plain = new_step(None, loss_t='uvem')
    ls0, _, _ = plain.step(*args_of(b, soft=True), 1e-3)
    torch.cuda.synchronize()
    assert torch.isfinite(ls).all() and torch.isfinite(lt).all() and not torch.equal(ls, ls0)
    assert st.style_flag_value() == 0 and plain.style_flag_value() == 0 and plain.last_style is None


def test_with_dacs_and_strong_the_teacher_sees_the_clean_tile_and_the_mix_pastes_the_matched_pixels():
    from regda_amd import ops
    b = batch(64, 3)
    keep = {k: b[k].clone() for k in ('images_t', 'images_s', 'label_s', 'regs_t')}
    hs = style(8, prob=1.0)
    st = new_step(dacs(2), ema_decay=0.9, strong=strong(4), style=hs)
    plain = new_step(dacs(2), ema_decay=0.9, strong=strong(4))
    for s in (st, plain):
        s.keep_debug = True
        s.step(*args_of(b), 1e-3)
        torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(b[k], v), k + ' was written'
    assert torch.equal(st.last_soft_t, plain.last_soft_t), "the teacher's soft labels"
    assert torch.equal(st.last_mix_table, plain.last_mix_table) and np.array_equal(st.last_strong, plain.last_strong)
    src = matched(b, hs, st.last_style)
    assert torch.equal(st.debug['source_s'], src)
    # style, then mix, then strong: the student's tile is the strong augmentation of the target tile with the MATCHED
    # source pixels pasted in
    mixed = ops.domain_mix_table(src, b['label_s'], st.last_mix_table, ops.MIX_CLASS, images_in=b['images_t'],
                                 images_out=torch.empty_like(b['images_t']), class_num=C)[0]
    clean_mix = ops.domain_mix_table(b['images_s'], b['label_s'], st.last_mix_table, ops.MIX_CLASS, images_in=b['images_t'],
                                     images_out=torch.empty_like(b['images_t']), class_num=C)[0]
    assert not torch.equal(mixed, clean_mix) and not torch.equal(mixed, b['images_t'])
    table = ops.strong_write_table(torch.empty(2, 8, device='cuda'), st.last_strong, (64, 64))
    sa = st.strong
    assert torch.equal(st.debug['student_t'], ops.strong_augment(mixed, table, sa.mean, sa.std))
    assert not torch.equal(st.debug['student_t'], plain.debug['student_t'])
    assert st.style_flag_value() == 0 and st.mix_flag_value() == 0 and st.strong_flag_value() == 0


def test_probability_zero_is_the_step_without_the_option_bit_for_bit():
    b = batch(64, 21)
    outs = []
    for s in (new_step(dacs(5), ema_decay=0.9, style=style(6, prob=0.0)), new_step(dacs(5), ema_decay=0.9)):
        o = s.step(*args_of(b), 1e-3)
        torch.cuda.synchronize()
        outs.append((o[0].clone(), o[1].clone(), o[2].clone(), s.last_hard.clone(), s.model.flat_p.clone(),
                     s.teacher.flat_p.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*outs))


def run_steps(seq, use_plan=False, st=None, which=None, seed=13):
    st = st if st is not None else new_step(dacs(seed), ema_decay=0.9, strong=strong(seed + 1), style=style(seed + 2))
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
                        mix=st.last_mix_table.clone(), strong=torch.from_numpy(st.last_strong.copy()),
                        style=torch.from_numpy(st.last_style.copy())))
    return st, out


def same_state(a, b):
    return (torch.equal(a.model.flat_p, b.model.flat_p) and torch.equal(a.model.flat_buf, b.model.flat_buf)
            and torch.equal(a.teacher.flat_p, b.teacher.flat_p) and torch.equal(a.mom, b.mom)
            and torch.equal(a.prototypes, b.prototypes))


def test_eager_steps_and_a_recorded_plan_give_the_same_bits_and_capture_refuses():
    """Eager, and one eager step + record_plan on the second + two replays: losses, masks, tables and weights bit for bit;
    the draw is a host action of the plan, so every replay draws afresh."""
    seq = [batch(64, 21), batch(64, 21), batch(64, 22), batch(64, 21)]
    st_a, out_a = run_steps(seq)
    st_p, out_p = run_steps(seq, use_plan=True)
    assert st_p._plan is not None and st_a._plan is None
    for i, (x, y) in enumerate(zip(out_a, out_p)):
        for k in x:
            assert torch.equal(x[k], y[k]), 'plan, step %d: %s differs' % (i, k)
    assert same_state(st_a, st_p)
    assert len({tuple(o['style'].flatten().tolist()) for o in out_p}) > 2      # a replay re-runs the draw
    assert st_p.style_flag_value() == 0
    with pytest.raises(RuntimeError, match='record_plan'):
        st_a.capture(*args_of(seq[0]))
    only = new_step(None, ema_decay=0.9, style=style(1))
    only.step(*args_of(seq[0]), 1e-3)
    with pytest.raises(RuntimeError, match=r'style=.*record_plan'):
        only.capture(*args_of(seq[0]))


def test_resume_after_step_two_of_four_continues_the_draws(tmp_path):
    from regda_amd.checkpoint import load_training_state, save_training_state
    seq = [batch(64, 21), batch(64, 22), batch(64, 21), batch(64, 22)]
    torch.manual_seed(77)
    a, out_a = run_steps(seq, seed=31)
    torch.manual_seed(77)
    b, _ = run_steps(seq, which=range(2), seed=31)
    assert 'style' in b.state_dict() and 'style' not in new_step(None).state_dict()
    path = str(tmp_path / 'style.pth')
    save_training_state(path, b, 2)
    c = new_step(dacs(99), init_seed=13, proto_seed=6, ema_decay=0.9, strong=strong(98), style=style(97))
    torch.manual_seed(5)
    assert load_training_state(path, c) == 2
    _, out_c = run_steps(seq, st=c, which=range(2, 4))
    for i, (x, y) in enumerate(zip(out_a[2:], out_c)):
        for k in x:
            assert torch.equal(x[k], y[k]), 'step %d: %s differs' % (i + 2, k)
    assert same_state(a, c)
    # a state with 'style' and a step without one, and the other way round
    with pytest.raises(ValueError, match='style'):
        load_training_state(path, new_step(dacs(1), ema_decay=0.9, strong=strong(2)))
    without = str(tmp_path / 'plain.pth')
    save_training_state(without, new_step(dacs(1), ema_decay=0.9), 0)
    with pytest.raises(ValueError, match='style'):
        load_training_state(without, new_step(dacs(1), ema_decay=0.9, style=style(2)))


def model(images):
    """the shallow model with dropout switched off for a forward of `images` tiles"""
    m = build()
    m.load_state_dict(init_sd(12), strict=True)
    m.set_drop_masks(torch.ones(images, 512), torch.ones(images, 512))
    return m


def test_the_source_and_the_align_step_take_style():
    from regda_amd.align import AlignStep
    from regda_amd.source import SourceStep
    b = batch(64, 3)
    keep = {k: b[k].clone() for k in ('images_t', 'images_s', 'label_s', 'regs_t')}
    hs = style(3, prob=1.0)
    src = SourceStep(model(2), style=hs)       # stage 1 forwards the source tiles alone
    src.keep_debug = True
    with pytest.raises(ValueError, match='target images'):
        src.step(b['images_s'], b['label_s'], None, 1e-3)
    assert src.last_style is None and src.first          # refused before anything ran
    loss, _, gn = src.step(b['images_s'], b['label_s'], b['images_t'], 1e-3)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(gn).all() and torch.isfinite(src.model.flat_p).all()
    assert torch.equal(src.debug['source_s'], matched(b, hs, src.last_style))
    plain = SourceStep(model(2))
    loss0, _, _ = plain.step(b['images_s'], b['label_s'], None, 1e-3)
    torch.cuda.synchronize()
    assert not torch.equal(loss, loss0) and 'style' in src.state_dict() and 'style' not in plain.state_dict()
    protos = torch.randn(C, 2048, generator=torch.Generator().manual_seed(5))
    ha = style(9, prob=1.0)
    al = AlignStep(model(4), protos, style=ha)
    al.keep_debug = True
    loss, la, gn = al.step(b['images_s'], b['label_s'], b['images_t'], b['regs_t'], 1e-3)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(la).all() and torch.isfinite(gn).all()
    assert torch.equal(al.debug['source_s'], matched(b, ha, al.last_style))
    for k, v in keep.items():
        assert torch.equal(b[k], v), k + ' was written'
    assert src.style_flag_value() == 0 and al.style_flag_value() == 0
