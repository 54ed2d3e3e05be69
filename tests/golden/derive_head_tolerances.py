"""Derive the per-element bounds of tests/test_align_passes_gpu.py and tests/test_teacher_passes_gpu.py for their float
outputs.  Runs on the CPU:
    python tests/golden/derive_head_tolerances.py
Per case it measures the largest per-element deviation of an fp32 oracle from the fp64 reference on the same inputs --
what fp32 arithmetic ALONE does to these numbers on these inputs.  A correct fp32 kernel is another realisation of that
rounding noise, so its bound is margin * deviation with margin 3, the margin of tests/golden/derive_label_tolerances.py.
No number measured on a GPU enters.

  pcl     oracle.labelpath.prototype_contrastive_loss in fp32 with autograd (labels outside [0, C) mapped to ignore first,
          as the kernel drops them; weight and the loss already in the tensor applied in fp32) against
          align_cases.pcl_ref.  `loss`: the scalar.  `grad`: every gradient element; the test adds the analytic bf16
          storage term 2^-8 |ref| (2^-8 |old + ref| when accumulating) per element itself.  zero_feature_pixel: the
          degenerate pixel's row (values of order 1e10) is measured and bounded on its own, `grad_row`, so that it does
          not widen the bound of the other rows.  The cases with NaN / Inf features: the rows of the other pixels,
          measured with the non-finite features replaced by 0 (the per-pixel gradients do not depend on each other,
          only on the kept count); their loss is NaN and has no bound.
  dbias   an fp32 numpy sum added to the pre-filled fp32 value, against align_cases.dbias_ref in fp64.
  resize  F.interpolate(bilinear, align_corners=True) in fp32 against teacher_cases.resize_ref.

Where a deviation comes out as exactly zero the bound is the floor FLOOR_ULPS * 2^-24 * max |reference| instead (a few
fp32 roundings at the output's scale), recorded as "floor": true.  Writes head_tolerances.json."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import align_cases as A  # noqa: E402
import teacher_cases as T  # noqa: E402
from oracle import labelpath as opath  # noqa: E402

MARGIN = 3.0
FLOOR_ULPS = 4.0


def entry(dev, scale):
    floor = dev == 0.0
    return dict(deviation=dev, bound=(FLOOR_ULPS * 2.0 ** -24 * scale) if floor else MARGIN * dev, floor=floor)


def pcl_oracle32(x, case):
    """-> (loss f32 scalar incl. loss0, grad (b, hw, K) f32) from the fp32 oracle with autograd."""
    feat = torch.from_numpy(x['feat']).clone().requires_grad_(True)
    lab = torch.from_numpy(x['lab']).clone()
    lab[(lab != case.ignore) & ((lab < 0) | (lab >= case.C))] = case.ignore
    loss = opath.prototype_contrastive_loss(torch.from_numpy(x['protos']), feat, lab, case.temp, case.ignore)
    loss = torch.tensor(case.weight, dtype=torch.float32) * loss
    loss.backward()
    total = torch.tensor(case.loss0, dtype=torch.float32) + loss.detach()
    b, K = feat.shape[:2]
    return float(total), feat.grad.reshape(b, K, -1).permute(0, 2, 1).numpy()


def pcl_entries(case):
    x = A.pcl_inputs(case)
    bad = ~np.isfinite(x['feat'].reshape(case.b, case.K, -1)).all(1)                   # (b, hw)
    healed = bool(bad.any())
    x['feat'][~np.isfinite(x['feat'])] = 0.0
    loss64, grad64, _, _ = A.pcl_ref(x['feat'], x['protos'], x['lab'], case.temp, case.ignore, case.weight)
    loss32, grad32 = pcl_oracle32(x, case)
    d = np.abs(grad32.astype(np.float64) - grad64)
    out = {}
    rows = ~bad
    if case.special == 'zero_pixel':
        rows[0, A.DEGENERATE_PIXEL] = False
        out['grad_row'] = entry(float(d[~rows].max()), float(np.abs(grad64[~rows]).max()))
    if not healed:
        out['loss'] = entry(abs(loss32 - (case.loss0 + loss64)), abs(case.loss0 + loss64))
    out['grad'] = entry(float(d[rows].max()), float(np.abs(grad64[rows]).max()))
    return out


def main():
    pcl = {c.name: pcl_entries(c) for c in A.PCL_CASES if 'none_kept' not in c.paths}
    dbias = {}
    for c in A.ASPP_CASES:
        x = A.aspp_inputs(c)
        r64 = np.stack(A.dbias_ref(x['g1'], x['g2'], x['dbias0']))
        r32 = np.stack(A.dbias_ref(x['g1'], x['g2'], x['dbias0'], np.float32))
        dbias[c.name] = entry(float(np.abs(r32.astype(np.float64) - r64).max()), float(np.abs(r64).max()))
    resize = {}
    for shape, size in T.RESIZE_CASES:
        x = T.resize_inputs(shape, size)
        r64 = T.resize_ref(x, size)
        resize[T.resize_name(shape, size)] = entry(float((T.resize_oracle32(x, size).double() - r64).abs().max()),
                                                   float(r64.abs().max()))
    out = dict(margin=MARGIN, floor_ulps=FLOOR_ULPS, pcl=pcl, dbias=dbias, resize=resize,
               rule='bound = margin * max |fp32 oracle - fp64 reference| on the case (CPU); floor_ulps * 2^-24 * max |reference| '
                    'where that deviation is exactly 0')
    with open(os.path.join(HERE, 'head_tolerances.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
