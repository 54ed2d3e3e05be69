"""dev: the fused --ls / --lt losses (rgda_upsample_loss; GDPLoss: rgda_upsample_gdp, plain and with the prototype and
class weights) against the CE call (rgda_upsample_ce) at 8 x 6 x 32 x 32 -> 512 x 512 (HIP-event time per loss_calc
call, with gradients; algorithmic bytes), rgda_proto_pixel_weight with and without a precomputed similarity map, and
IAST's regularisers (rgda_upsample_reg: derived masks, both terms, gradients accumulated) and adaptive pseudo-label
stages (rgda_iast_hist / _percentile / _label at 8 x 6 x 512 x 512, random and all-confident probabilities), and
the step time of SSLStep(loss_t='uvem' / 'ohem' / 'ghm' / 'gdp') and of SSLStep(ent_weight, kld_weight) ('reg') against
the default, as bench.py builds it (ResNet-101, 8 + 8 images, recorded plan; --eager: eager steps).
    python scripts/dev/loss_bench.py [--no-step] [--eager] [--only ghm,gdp,reg,iast]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from regda_amd import ops


def t_of(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def loss_calls():
    g = torch.Generator().manual_seed(0)
    b, c, h, H = 8, 6, 32, 512
    p1, p2 = (torch.randn(b, c, h, h, generator=g) * 2).cuda(), (torch.randn(b, c, h, h, generator=g) * 2).cuda()
    lab = torch.randint(-1, c, (b, H, H), generator=g).cuda()
    # confident labels: OHEM takes the top-k (radix select) branch
    base = torch.randn(b, c, h, h, generator=g) * 24
    q1, q2 = (base + 0.2 * torch.randn(b, c, h, h, generator=g)).cuda(), (base + 0.2 * torch.randn(b, c, h, h, generator=g)).cuda()
    lab_c = torch.nn.functional.interpolate(base, (H, H), mode='bilinear', align_corners=True).argmax(1).cuda()
    soft = torch.softmax(torch.randn(b, c, H, H, generator=g) * 3, 1).cuda()
    g1, g2 = torch.empty_like(p1), torch.empty_like(p2)
    acc = torch.zeros(30, device='cuda')
    npix = b * H * H
    # algorithmic bytes: int64 labels (read by each pass), the soft label (ups / uvem), the per-pixel scratch written by
    # the stat pass and read by the gradient pass, low-res logits and gradients (2 heads)
    low = 2 * 2 * b * c * h * h * 4
    passes = {'ce': 1, 'focal': 1}       # (reg: the count pass and the row pass, 2)
    scratch = {'ohem': 2 * npix * 4, 'ghm': 2 * npix, 'gdp': 2 * npix, 'ups': npix * 4, 'uvem': npix * 4}
    bw = torch.zeros(30, device='cuda')
    acc_gdp = torch.zeros(30, device='cuda')
    pw = torch.rand(npix, generator=g).cuda()
    cw = torch.rand(2, c, generator=g).cuda()
    feat = torch.randn(b, 2048, h, h, generator=g).cuda()
    protos = torch.randn(c, 2048, generator=g).cuda()
    _, _, sim = ops.label_refine(feat, protos, p1, p2, soft, 2.0, return_ws=True, return_sim=True)
    pw_out = torch.empty(npix, device='cuda')
    runs = [('ce', lambda: ops.upsample_ce(p1, p2, lab, -1, None, True, g1, g2))]
    kw = dict(thresh=0.35667494, momentum=0.99, g1=g1, g2=g2)
    runs += [('ohem', lambda: ops.upsample_loss('ohem', p1, p2, lab, **kw)),
             ('ohem top-k', lambda: ops.upsample_loss('ohem', q1, q2, lab_c, **kw)),
             ('focal', lambda: ops.upsample_loss('focal', p1, p2, lab, gamma=2.0, **kw)),
             ('ghm', lambda: ops.upsample_loss('ghm', p1, p2, lab, acc_sum=acc, **kw)),
             ('ups', lambda: ops.upsample_loss('ups', p1, p2, lab, soft=soft, t=0.7, **kw)),
             ('uvem', lambda: ops.upsample_loss('uvem', p1, p2, lab, soft=soft, m=0.2, t=0.7, gamma=4.0, **kw)),
             ('gdp', lambda: ops.upsample_gdp(p1, p2, lab, acc_gdp, bw, g1=g1, g2=g2)),
             ('gdp +pw+cw', lambda: ops.upsample_gdp(p1, p2, lab, acc_gdp, bw, pixel_weight=pw, class_weight=cw, g1=g1,
                                                     g2=g2)),
             ('reg', lambda: ops.upsample_reg(p1, p2, lab, lambda_ent=0.3, lambda_kld=0.1, g1=g1, g2=g2, accumulate=True,
                                              empty_is_zero=True))]
    only = sys.argv[sys.argv.index('--only') + 1].split(',') if '--only' in sys.argv else None
    if only:
        runs = [r for r in runs if r[0] == 'ce' or r[0].split()[0] in only]
    t_ce = None
    for name, fn in runs:
        t = t_of(fn)
        t_ce = t if t_ce is None else t_ce
        k = name.split()[0]
        nbytes = passes.get(k, 2) * npix * 8 + 2 * scratch.get(k, 0) + low + (c * npix * 4 if k in ('ups', 'uvem') else 0)
        nbytes += 2 * npix * 4 if name == 'gdp +pw+cw' else 0         # the prototype weights, read once per head
        print('%-11s %7.1f us  %.2fx CE   %6.1f MB algorithmic' % (name, t, t / t_ce, nbytes / 1e6), flush=True)
    if only is None or 'gdp' in only:
        for name, fn in (('proto_pixel_weight', lambda: ops.proto_pixel_weight(feat, protos, lab, out=pw_out)),
                         ('proto_pixel_weight sim=', lambda: ops.proto_pixel_weight(None, None, lab, sim=sim, out=pw_out))):
            print('%-24s %7.1f us' % (name, t_of(fn)), flush=True)
    if only is None or 'iast' in only:
        iast_stages(b, c, H, g)


def iast_stages(n, c, H, g):
    """The three stages of IASTSelector.update on random softmax probabilities and on all-confident ones (every pixel
    exactly 1.0: one histogram bin per class takes every add)."""
    conf = torch.zeros(n, c, H, H)
    conf.scatter_(1, torch.randint(0, c, (n, 1, H, H), generator=g), 1.0)
    inputs = (('uniform', torch.softmax(torch.randn(n, c, H, H, generator=g) * 3, 1).cuda()), ('confident', conf.cuda()))
    prepend = torch.full((c,), 0.9, dtype=torch.float64, device='cuda')
    q = torch.full((c,), 0.9139, dtype=torch.float64, device='cuda')
    out = torch.empty(n, H, H, dtype=torch.uint8, device='cuda')
    for name, probs in inputs:
        ws = ops.iast_workspace(n, c, H, H, probs.device)
        t_h = t_of(lambda: ops.iast_hist(probs, ws=ws))
        t_p = t_of(lambda: ops.iast_percentile(ws, prepend, q))
        t_l = t_of(lambda: ops.iast_label(ws, prepend, n, H, H, out=out))
        mb = probs.numel() * 4 / 1e6
        print('iast %-9s hist %7.1f us (%.0f MB of probabilities: %.2f TB/s)  percentile %6.1f us  label %6.1f us' %
              (name, t_h, mb, mb / t_h, t_p, t_l), flush=True)


def step_times():
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.ssl import SSLStep
    from regda_amd.synthetic import make_batch
    batch = make_batch(b=8, size=512, seed=2333, with_soft=True)
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(0))
    eager = '--eager' in sys.argv
    only = sys.argv[sys.argv.index('--only') + 1].split(',') if '--only' in sys.argv else ('none', 'uvem', 'ohem', 'ghm', 'gdp',
                                                                                          'reg')
    for lt in [k for k in ('none', 'uvem', 'ohem', 'ghm', 'gdp', 'reg') if k in only]:
        torch.manual_seed(2333)
        model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False),
                               multi_layer=True, cascade=False, use_ppm=True,
                               ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048, num_classes=6,
                               is_ins_norm=True))
        model.sync_weights()
        # 'reg': the default target loss + IAST's entropy and KLD terms
        st = SSLStep(model, protos, ent_weight=0.3, kld_weight=0.1) if lt == 'reg' else SSLStep(model, protos, loss_t=lt)
        args = (batch['images_s'], batch['label_s'], batch['images_t'], batch['soft_t'], batch['regs_t'])
        for _ in range(2):
            st.step(*args, 1e-3)
        if not eager:
            st.record_plan(*args)
        t = t_of(lambda: st.step(*args, 1e-3), reps=10) / 1e3
        print('SSLStep(loss_t=%r): %.2f ms per step (%s)' % (lt, t, 'eager' if eager else 'recorded plan'), flush=True)
        del st, model
        torch.cuda.empty_cache()


if __name__ == '__main__':
    loss_calls()
    if '--no-step' not in sys.argv:
        step_times()
