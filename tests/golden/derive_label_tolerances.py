"""Derive the per-element bounds of tests/test_label_passes_gpu.py for the float outputs of the label path.  Runs on the CPU:
    python tests/golden/derive_label_tolerances.py
Per case family it measures, over every case of tests/label_cases.py in the family, the largest per-element deviation
of the fp32 oracle (the same formula in torch fp32: oracle/labelpath.py, another summation order than the kernels') from
the fp64 reference on the same fp32 inputs -- what fp32 arithmetic ALONE does to these numbers on these inputs.  A
correct fp32 kernel is another realisation of that rounding noise, so its bound is margin * deviation with margin 3,
the margin of the project's other derived tolerances.  No number measured on a GPU enters.

Families: refine (label_refine / label_refine_views), refine_sup (label_refine_sup), teacher (teacher_probs),
proto_sums (the per-class feature sums of proto_stats; the counts are exact), protos (the prototypes after proto_apply
/ proto_update, decay 0.996 and 0).  Writes label_tolerances.json: margin, observed, bounds."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import label_cases as L  # noqa: E402
from oracle import labelpath as opath  # noqa: E402

MARGIN = 3.0
DECAYS = (0.996, 0.0)


def dev(a32, ref64):
    return float((a32.double() - ref64).abs().max())


def main():
    obs = dict(refine=0.0, refine_sup=0.0, teacher=0.0, proto_sums=0.0, protos=0.0)
    per_case = {}
    for c in L.REFINE_CASES:
        x = L.refine_inputs(c)
        a = (x['feat'], x['protos'], x['p1'], x['p2'], x['soft'], x['sup'], c.temp, c.views)
        d = dev(L.refine_oracle32(*a), L.refine_ref(*a))
        per_case['refine:' + c.name] = d
        fam = 'refine_sup' if c.sup else 'refine'
        obs[fam] = max(obs[fam], d)
    for i in range(len(L.TEACHER_CASES)):
        p1, p2, size = L.teacher_inputs(i)
        d = dev(opath.teacher_probs(p1, p2, size), L.teacher_ref(p1, p2, size))
        per_case['teacher:%d' % i] = d
        obs['teacher'] = max(obs['teacher'], d)
    for c in L.DS_CASES:
        label, feat, protos, _ = L.ds_inputs(c)
        feat, protos = torch.from_numpy(feat), torch.from_numpy(protos)
        ds = torch.from_numpy(L.downscale_ref(label, c.scale, c.C, -1, c.min_ratio)[0])
        s64, n64 = L.proto_sums_ref(feat, ds, c.C)
        s32, n32 = opath.prototype_statistics(feat, ds, c.C, -1)
        assert torch.equal(n32.double(), n64)
        d = dev(s32, s64)
        per_case['proto_sums:' + c.name] = d
        obs['proto_sums'] = max(obs['proto_sums'], d)
        for decay in DECAYS:
            d = dev(opath.apply_prototype_statistics(protos, s32, n32, decay), L.proto_apply_ref(protos, s64, n64, decay))
            per_case['protos:%s:%g' % (c.name, decay)] = d
            obs['protos'] = max(obs['protos'], d)
    out = dict(margin=MARGIN, observed=obs, bounds={k: MARGIN * v for k, v in obs.items()}, per_case=per_case,
               rule='bound = margin * max over the family\'s cases of max |fp32 oracle - fp64 reference| (CPU)')
    with open(os.path.join(HERE, 'label_tolerances.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
