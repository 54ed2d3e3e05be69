"""CPU: the state_dict / load_state_dict pairs of the host-side helpers a training script holds itself, and the file
helpers of regda_amd/checkpoint.py (atomic write, named entries).  The fused steps' own state is tested on the GPU
(tests/test_resume_gpu.py)."""
import os

import numpy as np
import pytest
import torch


class FakeStep:
    """Stands in for a fused step: plain state out, the same state back in."""

    def __init__(self, value):
        self.value = torch.full((3,), float(value))

    def state_dict(self):
        return {'format': 1, 'value': self.value.clone()}

    def load_state_dict(self, sd, strict=True):
        self.value = sd['value'].clone()


def reload(sd, tmp_path):
    """through a file read with weights_only=True, as a training script would"""
    path = os.path.join(tmp_path, 'sd.pth')
    torch.save(sd, path)
    return torch.load(path, weights_only=True)


@pytest.mark.parametrize('kind', ['class', 'box'])
@pytest.mark.parametrize('k', [0, 7])
def test_domain_mix_continues_its_draws(kind, k, tmp_path):
    from regda_amd.aug.mix import DomainMix
    a = DomainMix(kind, 6, prob=0.7, seed=5)
    for _ in range(k):
        a.draw(64, 48)
    sd = reload(a.state_dict(), tmp_path)
    expect = [a.draw(64, 48) for _ in range(20)]
    b = DomainMix(kind, 6, prob=0.7, seed=99)
    assert [DomainMix(kind, 6, prob=0.7, seed=99).draw(64, 48) for _ in range(20)] != expect
    b.load_state_dict(sd)
    assert [b.draw(64, 48) for _ in range(20)] == expect
    with pytest.raises(ValueError, match='rng'):
        b.load_state_dict({})
    with pytest.raises(ValueError, match='bit_generator'):
        b.load_state_dict({'rng': dict(sd['rng'], bit_generator='MT19937')})


def small_model(seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 2, 1))
    m[2].bias.requires_grad_(False)         # not averaged
    return m


def test_ema_round_trip_and_next_update(tmp_path):
    from regda_amd.utils.ema import ExponentialMovingAverage
    m = small_model(0)
    a = ExponentialMovingAverage(m, 0.9)
    a.register()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.25)
    a.update()
    sd = reload(a.state_dict(), tmp_path)
    assert set(sd['shadow']) == {n for n, p in m.named_parameters() if p.requires_grad} and '2.bias' not in sd['shadow']
    # a fresh object on the same (live) model, registered at other values and not registered at all
    for register in (True, False):
        b = ExponentialMovingAverage(m, 0.9)
        if register:
            b.register()
            held = dict(b.shadow)
        b.load_state_dict(sd)
        assert all(torch.equal(b.shadow[n], a.shadow[n]) for n in a.shadow)
        if register:
            assert all(b.shadow[n] is held[n] for n in held)        # copied into what the object holds
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)
    a.update()
    b.update()
    assert all(torch.equal(b.shadow[n], a.shadow[n]) for n in a.shadow)
    # refusals leave the shadow as it was
    before = {n: v.clone() for n, v in b.shadow.items()}
    bad = {'shadow': dict(sd['shadow'])}
    del bad['shadow']['0.weight']
    with pytest.raises(ValueError, match='0.weight'):
        b.load_state_dict(bad)
    bad = {'shadow': dict(sd['shadow'], **{'1.weight': torch.zeros(5)})}
    with pytest.raises(ValueError, match='1.weight'):
        b.load_state_dict(bad)
    assert all(torch.equal(b.shadow[n], before[n]) for n in before)


def test_iast_selector_thresholds_round_trip_in_float64(tmp_path):
    from regda_amd.utils.tools import IASTSelector
    a = IASTSelector(6, 0.2, 0.9, 8.0)
    a.cls_thresh = np.random.default_rng(3).random(6) * 0.5 + 0.4999999999999         # not representable in float32
    sd = reload(a.state_dict(), tmp_path)
    assert sd['cls_thresh'].dtype == torch.float64
    b = IASTSelector(6, 0.2, 0.9, 8.0)
    b.load_state_dict(sd)
    assert b.cls_thresh.dtype == np.float64 and b.cls_thresh.tobytes() == a.cls_thresh.tobytes()
    assert b.cls_thresh is not a.cls_thresh and np.array_equal(b.quantiles(), a.quantiles())
    with pytest.raises(ValueError, match='cls_thresh'):
        IASTSelector(7, 0.2, 0.9, 8.0).load_state_dict(sd)
    with pytest.raises(ValueError, match='cls_thresh'):
        b.load_state_dict({'cls_thresh': sd['cls_thresh'].float()})
    assert b.cls_thresh.tobytes() == a.cls_thresh.tobytes()


def test_a_failed_write_leaves_the_previous_file_whole(tmp_path, monkeypatch):
    from regda_amd import checkpoint
    path = os.path.join(tmp_path, 'state.pth')
    assert checkpoint.save_training_state(path, FakeStep(1), 10) is None
    good = open(path, 'rb').read()
    real_save = torch.save

    def failing_save(obj, f, *a, **k):
        f.write(b'half a file')          # the temporary file is open and partly written
        f.flush()
        raise OSError('no space left on device')
    monkeypatch.setattr(torch, 'save', failing_save)
    with pytest.raises(OSError, match='no space'):
        checkpoint.save_training_state(path, FakeStep(2), 20)
    monkeypatch.setattr(torch, 'save', real_save)
    assert open(path, 'rb').read() == good
    assert os.listdir(tmp_path) == ['state.pth']            # and no temporary file stays behind
    st = FakeStep(0)
    assert checkpoint.load_training_state(path, st) == 10 and torch.equal(st.value, torch.full((3,), 1.0))


def test_named_entries_of_the_file_and_of_the_call_must_match(tmp_path):
    from regda_amd import checkpoint
    from regda_amd.aug.mix import DomainMix
    from regda_amd.utils.tools import IASTSelector
    path = os.path.join(tmp_path, 'state.pth')
    mix, sel = DomainMix('class', 6, seed=1), IASTSelector(6)
    mix.draw(32, 32)
    checkpoint.save_training_state(path, FakeStep(4), 123, mix=mix, selector=sel)
    raw = torch.load(path, weights_only=True)
    assert sorted(raw) == ['format', 'iteration', 'mix', 'selector', 'step'] and raw['iteration'] == 123
    st, mix2 = FakeStep(0), DomainMix('class', 6, seed=2)
    for named in (dict(mix=mix2), dict(mix=mix2, selector=sel, more=sel), dict()):
        with pytest.raises(ValueError, match='named entries'):
            checkpoint.load_training_state(path, st, **named)
    assert torch.equal(st.value, torch.zeros(3))            # refused before anything was loaded
    assert checkpoint.load_training_state(path, st, mix=mix2, selector=sel) == 123
    assert torch.equal(st.value, torch.full((3,), 4.0)) and mix2.draw(32, 32) == mix.draw(32, 32)
    with pytest.raises(ValueError, match='reserved'):
        checkpoint.save_training_state(path, FakeStep(4), 1, format=mix)
    raw['format'] = 99
    torch.save(raw, path)
    with pytest.raises(ValueError, match='format'):
        checkpoint.load_training_state(path, st, mix=mix2, selector=sel)
