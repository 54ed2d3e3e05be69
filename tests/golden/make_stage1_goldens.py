"""Mint the stage-1 golden vectors from the reference's OWN Python (imported behind the same stubs as make_goldens.py).

Run in the build container only (needs the reference checkout):
    python tests/golden/make_stage1_goldens.py [coral] [proto_init] [src_small]
Writes coral.npz (CoralLoss / Aligner.align_domain: loss and autograd gradients), proto_init.npz (Aligner.update_avg
over three batches + init_avg, one class never present) and src_small.npz (one tools/train_src.py iteration with
--align-domain 1 on the ResNet-101 of model_small.npz).  Data only: inputs and the reference's outputs."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (installs the stubs, imports the reference)

from regda.gast.alignment import Aligner  # noqa: E402
from regda.gast.coral import CoralLoss  # noqa: E402
from regda.gast.balance import CrossEntropy  # noqa: E402
from regda.utils.tools import loss_calc  # noqa: E402

from oracle import model as omodel  # noqa: E402  (only for the seeded weight generator)


def _q(rng, shape, scale=32.0):
    """random features on a grid of 1/scale (stored as int8: exact in fp32, a small fixture)"""
    return np.clip(np.round(rng.standard_normal(shape) * scale * 0.8), -127, 127).astype(np.int8)


def gold_coral():
    """CoralLoss()(source, target) on (n, d) rows (two cases at d = 64, ns == nt and ns != nt) and
    Aligner.align_domain(feat_s, feat_t) on (b, 2048, h, w) maps of the model_small feature shape; forward + autograd."""
    rng = np.random.default_rng(1607)
    out = {}
    crit = CoralLoss()
    for i, (ns, nt, d) in enumerate(((96, 96, 64), (80, 144, 64))):
        qs, qt = _q(rng, (ns, d)), _q(rng, (nt, d))
        # a domain shift in mean and scale so that D is not only noise
        xs = torch.from_numpy(qs.astype(np.float32) / 32.0).requires_grad_(True)
        xt = torch.from_numpy(qt.astype(np.float32) / 32.0 * 1.5 + 0.25).requires_grad_(True)
        loss = crit(xs, xt)
        loss.backward()
        out.update({f'qs{i}': qs, f'qt{i}': qt, f'loss{i}': loss.detach().numpy(), f'gs{i}': xs.grad.numpy(),
                    f'gt{i}': xt.grad.numpy()})
    al = Aligner(logger=mg._Log(), feat_channels=2048, class_num=6, ignore_label=-1, decay=0.999, resume=None)
    shape = (2, 2048, 4, 4)
    qs, qt = _q(rng, shape), _q(rng, shape)
    fs = torch.from_numpy(qs.astype(np.float32) / 32.0).requires_grad_(True)
    ft = torch.from_numpy(qt.astype(np.float32) / 32.0 * 1.25).requires_grad_(True)
    loss = al.align_domain(fs, ft)
    loss.backward()
    out.update(qs2=qs, qt2=qt, loss2=loss.detach().numpy(), gs2=fs.grad.numpy(), gt2=ft.grad.numpy())
    out['scales'] = np.array([[1.0, 1.5, 0.25], [1.0, 1.5, 0.25], [1.0, 1.25, 0.0]], np.float32)   # xt = q/32 * s + o
    mg.save('coral.npz', **out)


def gold_proto_init():
    """Aligner.update_avg over three (feat, label) batches then init_avg (alignment.py:107-126), 64 channels; labels in
    {-1, 0 .. 4}: class 5 never occurs (its prototype is 0)."""
    rng = np.random.default_rng(2023)
    al = Aligner(logger=mg._Log(), feat_channels=64, class_num=6, ignore_label=-1, decay=0.996, resume=None)
    out = {}
    for i in range(3):
        feat = rng.standard_normal((2, 64, 4, 4)).astype(np.float32)
        # blocky labels so the 16x downscale keeps classes (min_ratio 0.75) and some cells are mixed (-> ignored)
        cells = rng.integers(-1, 5, (2, 4, 4))
        lab = np.repeat(np.repeat(cells, 16, 1), 16, 2)
        noise = rng.random(lab.shape) < 0.2
        lab = np.where(noise, rng.integers(-1, 5, lab.shape), lab).astype(np.int8)
        al.update_avg(torch.from_numpy(feat), torch.from_numpy(lab.astype(np.int64)))
        out[f'feat{i}'], out[f'lab{i}'] = feat, lab
    al.init_avg()
    out.update(data_sum=al._data_sum.numpy(), data_cnt=al._data_cnt.numpy(), protos=al.prototypes.numpy())
    mg.save('proto_init.npz', **out)


def gold_src_small():
    """One stage-1 iteration on the reference model, composed exactly like tools/train_src.py:117-140 with
    --align-domain 1 (CrossEntropy, no class balancer): model(xs), model(xt), loss_calc + align_domain, backward.
    Same inputs and weights as model_small.npz; the Dropout2d keep-masks of the two forwards are captured."""
    src = np.load(os.path.join(HERE, 'model_small.npz'))
    m = mg.build_ref_model()
    sd = omodel.init_state_dict('resnet101', 6, seed=1)
    m.load_state_dict(sd, strict=True)
    m.train()
    masks = {}

    def hook(name):
        def fn(mod, inp, out):
            i, o = inp[0].detach(), out.detach()
            keep = ((o != 0).flatten(2).any(-1) | (i == 0).flatten(2).all(-1))
            masks.setdefault(name, []).append(keep.numpy().astype(np.uint8))
        return fn
    m.layer5.conv_last[3].register_forward_hook(hook('m5'))
    m.layer6.conv_last[3].register_forward_hook(hook('m6'))
    xs, xt = torch.from_numpy(src['xs']), torch.from_numpy(src['xt'])
    lab_s = torch.from_numpy(src['lab_s'].astype(np.int64))
    al = Aligner(logger=mg._Log(), feat_channels=2048, class_num=6, ignore_label=-1, decay=0.99, resume=None)
    ce = CrossEntropy(ignore_label=-1, class_balancer=None)
    torch.manual_seed(78)
    s1, s2, fs = m(xs)
    _, _, ft = m(xt)
    loss_seg = loss_calc([s1, s2], lab_s, loss_fn=ce, multi=True)
    loss_domain = al.align_domain(fs, ft)
    loss = loss_seg + loss_domain
    loss.backward()
    named = dict(m.named_parameters())
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in named.values() if p.grad is not None)).item()
    sel = ['encoder.resnet.conv1.weight', 'encoder.resnet.bn1.bias', 'layer5.conv_last.4.weight',
           'encoder.resnet.layer4.2.bn3.bias']
    grads = {('grad:' + k): named[k].grad.numpy() for k in sel}
    grads['grad:encoder.resnet.layer4.2.conv3.weight[:8]'] = named['encoder.resnet.layer4.2.conv3.weight'].grad[:8].numpy()
    mg.save('src_small.npz', m5=np.stack(masks['m5']), m6=np.stack(masks['m6']), loss_seg=loss_seg.detach().numpy(),
            loss_domain=loss_domain.detach().numpy(), grad_norm=np.float64(gn), **grads)


if __name__ == '__main__':
    for w in sys.argv[1:] or ['coral', 'proto_init', 'src_small']:
        globals()['gold_' + w]()
