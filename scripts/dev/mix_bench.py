"""rgda_domain_mix at the training shape (8 + 8 tiles of 512 x 512, C = 6; image, soft label and region map of the
target rewritten): class mode with int(C * 0.5) = 3 classes chosen over the block-constant synthetic labels, and a box
of half the tile's area.  One warm-up, then the median HIP-event time of `calls` calls; the bytes the predicate actually
moves (include/rgda_hip.h: 8 B of label per pixel that is read, and per pasted pixel 12 B read + 12 B written of image,
4 C of soft planes, 8 of region map) and the GB/s over that floor; the result is checked against tests/mix_ref.py.
    python scripts/dev/mix_bench.py [calls] [out.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mix_ref  # noqa: E402
from regda_amd import ops  # noqa: E402
from regda_amd.synthetic import make_batch  # noqa: E402

N, S, C = 8, 512, 6


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    b = make_batch(b=N, size=S, classes=C, seed=2333)
    classes = (0, 2, 4)
    half = int(round(S / np.sqrt(2)))
    box = ((S - half) // 2, (S - half) // 2 + half, (S - half) // 2, (S - half) // 2 + half)
    lines = []
    for name, pred in (('class %s' % (classes,), dict(classes=classes)), ('box %s' % (box,), dict(box=box))):
        t = {k: v.clone() for k, v in b.items()}
        args = (t['images_s'], t['label_s'], t['images_t'])
        kw = dict(soft_t=t['soft_t'], regs_t=t['regs_t'], class_num=C, **pred)
        ops.domain_mix(*args, **kw)                             # the warm-up; the call is idempotent
        torch.cuda.synchronize()
        want = mix_ref.domain_mix(*(b[k].cpu().numpy() for k in ('images_s', 'label_s', 'images_t')),
                                  soft_t=b['soft_t'].cpu().numpy(), regs_t=b['regs_t'].cpu().numpy(), C=C, **pred)
        same = all(mix_ref.bits_equal(t[k].cpu().numpy(), w) for k, w in zip(('images_t', 'soft_t', 'regs_t'), (want[0], want[2], want[3])))
        cond = want[5]
        times = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.domain_mix(*args, **kw)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        us = float(np.median(times))
        pasted = int(cond.sum())
        read = cond.size if 'classes' in pred else pasted       # box mode reads the labels inside the box only
        by = 8 * read + pasted * (24 + 4 * C + 8)
        lines.append('rgda_domain_mix %d x %d x %d, C %d, %s: %.1f %% pasted; median of %d calls %.1f us (min %.1f, max %.1f); '
                     'bytes moved %.1f MB -> %.0f GB/s over that floor; bit-identical to tests/mix_ref.py: %s'
                     % (N, S, S, C, name, 100.0 * pasted / cond.size, calls, us, min(times), max(times), by / 1e6,
                        by / us / 1e3, same))
    print('\n'.join(lines))
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
