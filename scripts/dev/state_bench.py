"""What a checkpoint of the training state costs: ResNet-101 with the online EMA teacher, two steps on
2 + 2 tiles of 128 x 128 (the state's size does not depend on the tiles), then the wall time of `step.state_dict()`
(device synchronise + every tensor to the host), of `save_training_state` to a file in `dir` (default: the system's
temporary directory) and of `load_training_state` back into the same step; median of `calls` calls each, the file's size,
and a check that the reloaded state is the saved one.
    python scripts/dev/state_bench.py [calls] [dir] [out.txt]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd.checkpoint import load_training_state, save_training_state  # noqa: E402
from regda_amd.models.Encoder import Deeplabv2  # noqa: E402
from regda_amd.ssl import SSLStep  # noqa: E402
from regda_amd.synthetic import make_batch  # noqa: E402


def wall(fn, calls):
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), min(times), max(times)


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    where = sys.argv[2] if len(sys.argv) > 2 else tempfile.gettempdir()
    torch.manual_seed(0)
    m = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False), multi_layer=True,
                       cascade=False, use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048,
                       num_classes=6, is_ins_norm=True))
    st = SSLStep(m, torch.randn(6, 2048), ema_decay=0.999)
    b = make_batch(b=2, size=128, seed=1, with_soft=False)
    for _ in range(2):
        st.step(b['images_s'], b['label_s'], b['images_t'], None, b['regs_t'], 1e-3)
    path = os.path.join(where, 'state_bench.%d.pth' % os.getpid())
    try:
        t_sd = wall(st.state_dict, calls)
        t_save = wall(lambda: save_training_state(path, st, 2), calls)
        size = os.path.getsize(path)
        before = st.state_dict()
        t_load = wall(lambda: load_training_state(path, st), calls)
        after = st.state_dict()
        same = all(torch.equal(before[k][n], after[k][n]) for k in ('model', 'teacher') for n in before[k]) and \
            torch.equal(before['mom'], after['mom']) and torch.equal(before['prototypes'], after['prototypes'])
    finally:
        if os.path.exists(path):
            os.unlink(path)
    line = ('training state, ResNet-101 + EMA teacher: %d parameters, file %.1f MB; median of %d calls (min, max): state_dict() '
            '%.0f ms (%.0f, %.0f); save_training_state %.0f ms (%.0f, %.0f); load_training_state %.0f ms (%.0f, %.0f); reloaded '
            'state identical: %s' % (m.flat_p.numel(), size / 1e6, calls, *t_sd, *t_save, *t_load, same))
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
