"""Derive the bounds of tests/test_loss_passes_gpu.py for the upsample-loss kernels.  Runs on the CPU:
    python tests/golden/derive_loss_tolerances.py
Per case of tests/loss_cases.py and per output (loss, g1, g2, GHM's acc_sum at a momentum above 0) it measures the
deviation of the fp32 restatement (tests/loss_ref.py, torch fp32 on the CPU: another summation order and other
transcendentals than the kernels') from the float64 reference on that case's inputs -- what fp32 arithmetic ALONE does to
these numbers.  A correct fp32 kernel is another realisation of that rounding noise, so its bound is
    margin * deviation + floor,   margin 3 (the margin of the project's other derived tolerances),
    floor = the number of terms in the longest sum * 2^-24 * the largest term
(a gradient element: the output pixels in a low-res pixel's footprint, the largest |d loss / d upsampled logit|; the loss:
every pixel, the largest per-pixel term; acc_sum: the three terms of the two EMA steps, the largest bin).  The loss is
relative, the others absolute and per element.  No number measured on a GPU enters.

Writes loss_tolerances.json: margin, rule, and per case observed / floor / bound."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import loss_cases as L  # noqa: E402

RULE = 'bound = margin * |fp32 restatement - fp64 reference| (CPU, this case) + terms * 2^-24 * largest term'


def derive(name):
    obs, floor = L.deviations(L.inputs(name))
    return dict(observed=obs, floor=floor, bound=L.bounds(obs, floor))


def main():
    out = dict(margin=L.MARGIN, rule=RULE, cases={c.name: derive(c.name) for c in L.CASES})
    with open(os.path.join(HERE, 'loss_tolerances.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    worst = {}
    for name, d in out['cases'].items():
        for k, v in d['bound'].items():
            key = (L.BY_NAME[name].kind, k[0])
            worst[key] = max(worst.get(key, 0.0), v)
    print(json.dumps({'%s:%s' % k: v for k, v in sorted(worst.items())}, indent=1))


if __name__ == '__main__':
    main()
