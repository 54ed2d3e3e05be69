"""Derive clan_tolerances.json on the CPU: no bound of the CLAN tests is fixed by hand.

    python tests/golden/derive_clan_tolerances.py

For every case the GPU tests run (tests/clan_ref.py holds the cases and draws their inputs) one bound per tensor, by
adv_ref's convention: three times the deviation of the bf16 storage model from float64 on the same case -- only P is
stored as bf16 by these kernels, everything else stays f32, so for the other tensors that term is 0 -- plus K * 2^-24 for
the f32 operations behind an element.  K, and the allowance for expf / log1pf (1 ULP each: the single-precision rows of
the HIP math accuracy table, "HIP math API" in the ROCm documentation), are worked out in clan_ref's docstring and its
*_tolerances functions."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clan_ref as C  # noqa: E402

PATH = os.path.join(HERE, 'clan_tolerances.json')


def derive():
    out = dict(margin=3.0, ulp_expf=C.ULP_EXPF, ulp_log1pf=C.ULP_LOG1PF, pair={}, wbce={}, golden={})
    for n in C.PAIR_CASES:
        c = C.pair_case(n)
        out['pair'][n] = C.pair_tolerances(c, C.pair_reference(c))
    for s in C.WBCE_SHAPES:
        c = C.wbce_case(s)
        for v in C.wbce_variants(s):
            t, use_w = v[0], v[1]
            if C.bounds_key(s, v) in out['wbce']:
                continue
            out['wbce'][C.bounds_key(s, v)] = C.wbce_tolerances(
                c['z'], c['size'], c['target'] if t == 'tensor' else t, c['wmap'] if use_w else None, C.ALPHA, C.BETA,
                C.wbce_reference(c, v))
    load = lambda fn: np.load(os.path.join(HERE, fn), allow_pickle=False)      # noqa: E731
    for n in C.GOLDEN_CASES:
        out['golden'][n] = C.golden_tolerances(C.golden_case(load, n))
    return out


if __name__ == '__main__':
    tol = derive()
    json.dump(tol, open(PATH, 'w'), indent=1, sort_keys=True)
    for group in ('pair', 'wbce', 'golden'):
        for n, t in tol[group].items():
            print(group, n, {k: '%.2e' % v for k, v in t.items()})
    print('wrote', PATH)
