"""CPU: the table of optional stage-2 loss terms (regda_amd.align.TERMS) -- its order, which is the order in which the
terms add onto the bf16 gradient rows and so part of the step's result, and the refusals the constructor makes before it
touches the model (no GPU, no library)."""
import pytest


def test_the_order_of_the_terms():
    from regda_amd.align import TERMS
    assert [t.name for t in TERMS] == ['domain', 'whiten', 'contrast', 'triplet', 'dca', 'saw', 'adv']


def test_every_weight_keyword_refuses_a_negative_value_before_the_model_is_touched():
    from regda_amd.align import TERMS, AlignStep
    keywords = [t.on for t in TERMS if t.on.endswith('_weight')]
    assert keywords == ['whiten_weight', 'contrast_weight', 'triplet_weight', 'dca_weight', 'saw_weight', 'adv_weight']
    for kw in keywords:
        for w in (-1.0, -1e-3):
            with pytest.raises(ValueError, match=f'AlignStep: {kw} must be >= 0'):
                AlignStep(None, None, **{kw: w})


def test_the_iast_regularisers_are_still_refused():
    from regda_amd.align import AlignStep
    with pytest.raises(NotImplementedError, match='ent_weight'):
        AlignStep(None, None, ent_weight=0.1)
    with pytest.raises(NotImplementedError, match='kld_weight'):
        AlignStep(None, None, kld_weight=0.1)
