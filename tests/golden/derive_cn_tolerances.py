"""Step-level tolerances of the class-count GPU tests (tests/test_class_counts_gpu.py), by the rule of
derive_tolerances.py: N = |bf16-emulating CPU oracle step - fp32 CPU oracle step| on the fixture, tolerance =
max(3 N, floor).  The functions are derive_tolerances.py's own (imported); the fixture is derive_c7_tolerances.py's at
16 classes, the widest count served.

Writes tests/golden/cn_tolerances.json.  Run in the build container (CPU only):
    python tests/golden/derive_cn_tolerances.py"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from derive_tolerances import cosine, noise  # noqa: E402
from oracle import model as omodel  # noqa: E402
from oracle.step import CpuStep  # noqa: E402
from regda_amd.synthetic import make_batch  # noqa: E402

C = 16


def shallow_cn_inputs(c=C):
    """resnet17t, seed 6, batch seed 11, 4 + 4 images of 128 x 128 with c-class labels and soft labels, all-ones dropout
    masks, lr 1e-3 (tests/test_class_counts_gpu.py::test_ssl_step_matches_the_oracle_step)."""
    rt = 'resnet17t'
    sd = omodel.init_state_dict(rt, c, seed=6)
    b = make_batch(b=4, size=128, classes=c, seed=11, device='cpu')
    protos = torch.randn(c, 2048, generator=torch.Generator().manual_seed(1))
    return rt, sd, b, protos, torch.ones(4, 512)


def shallow_cn_fixture():
    rt, sd, b, protos, ones = shallow_cn_inputs()
    res = []
    for emu in (False, True):
        cpu = CpuStep(sd, protos, resnet_type=rt, class_num=C, lr=1e-3, emulate_bf16=('grad' if emu else False))
        out = cpu.step(b['images_s'], b['label_s'], b['images_t'], b['soft_t'], b['regs_t'], (ones, ones), (ones, ones))
        res.append((out, cpu))
    (ref, cref), (emu, cemu) = res
    names = ['encoder.resnet.conv1.weight']
    n = noise(ref, emu, names)
    worst = {k: v for k, v in n.items() if not isinstance(v, dict)}
    worst['protos_rel'] = float((cemu.prototypes - cref.prototypes).norm() / cref.prototypes.norm())
    k = 'encoder.resnet.bn1.running_mean'
    worst['bn1_running_mean_abs'] = float((cemu.sd[k] - cref.sd[k]).abs().max())
    d_ref, d_emu = cref.sd[names[0]].detach() - sd[names[0]], cemu.sd[names[0]].detach() - sd[names[0]]
    worst['stem_update_cos'] = cosine(d_emu, d_ref)
    worst['stem_update_norm_dev'] = abs(float(d_emu.norm() / d_ref.norm()) - 1)
    return worst


if __name__ == '__main__':
    out = {'rule': 'tolerance = max(3 * N, floor); N = |bf16-emulating oracle - fp32 oracle| on the fixture (CPU); '
                   'cosines: 1 - tol_cos = 3 * (1 - N_cos)  (derive_tolerances.py)',
           'factor': 3.0,
           'shallow_step_c16': shallow_cn_fixture()}
    with open(os.path.join(HERE, 'cn_tolerances.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))
