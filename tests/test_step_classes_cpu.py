"""CPU: the shape of the step hierarchy (regda_amd/step.py) and the refusals the constructors make before they touch the
model (no GPU, no library): the stage-1 and stage-2 steps are not SSL steps, the SSL step's own options are refused by
name, and a keyword a step does not serve is an ordinary TypeError."""
import pytest


def classes():
    from regda_amd.align import AlignStep
    from regda_amd.source import SourceStep
    from regda_amd.ssl import SSLStep
    from regda_amd.step import FusedStep, PseudoLabelStep
    return FusedStep, PseudoLabelStep, SSLStep, AlignStep, SourceStep


def test_the_hierarchy():
    FusedStep, PseudoLabelStep, SSLStep, AlignStep, SourceStep = classes()
    assert not issubclass(SourceStep, SSLStep) and not issubclass(AlignStep, SSLStep)
    assert all(issubclass(c, FusedStep) for c in (SSLStep, AlignStep, SourceStep))
    assert issubclass(SSLStep, PseudoLabelStep) and issubclass(AlignStep, PseudoLabelStep)
    assert not issubclass(SourceStep, PseudoLabelStep)


def test_capture_and_record_plan_are_refused_in_one_place():
    FusedStep, _, SSLStep, AlignStep, SourceStep = classes()
    for name in ('capture', 'record_plan'):
        assert getattr(AlignStep, name) is getattr(SourceStep, name) is getattr(FusedStep, name)
        assert getattr(SSLStep, name) is not getattr(FusedStep, name)
        with pytest.raises(NotImplementedError, match='SSL step only'):
            getattr(FusedStep, name)(None)


@pytest.mark.parametrize('kw, match', [(dict(ent_weight=0.1), 'ent_weight'), (dict(kld_weight=0.1), 'kld_weight'),
                                       (dict(mix=object()), r'mix='), (dict(strong=object()), r'strong='),
                                       (dict(ema_decay=0.99), 'ema_decay')])
def test_the_options_of_the_ssl_step_are_refused_by_name(kw, match):
    *_, AlignStep, SourceStep = classes()
    for make in (lambda: AlignStep(None, None, **kw), lambda: SourceStep(None, **kw)):
        with pytest.raises(NotImplementedError, match=match) as e:
            make()
        assert 'SSL step' in str(e.value)


def test_switched_off_they_are_accepted():
    """ent_weight=0, mix=None, ... and ema_decay=None pass the refusal: the constructor gets as far as the model"""
    *_, AlignStep, SourceStep = classes()
    off = dict(ent_weight=0.0, kld_weight=0.0, mix=None, strong=None, ema_decay=None)
    for make in (lambda: AlignStep(None, None, **off), lambda: SourceStep(None, **off)):
        with pytest.raises(AttributeError, match='device'):
            make()


@pytest.mark.parametrize('step, kw', [('align', 'loss_t'), ('align', 'class_balancer_t'), ('align', 'uvem_m'),
                                      ('source', 'cutoff_top'), ('source', 'sam_refine'), ('source', 'proto_decay'),
                                      ('source', 'loss_t'), ('align', 'no_such_option'), ('source', 'no_such_option')])
def test_a_keyword_a_step_does_not_serve_is_a_type_error(step, kw):
    *_, AlignStep, SourceStep = classes()
    with pytest.raises(TypeError, match=kw):
        AlignStep(None, None, **{kw: 1}) if step == 'align' else SourceStep(None, **{kw: 1})
