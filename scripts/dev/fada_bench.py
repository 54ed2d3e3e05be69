"""The feature-adversarial path at b = 8 images of 512 x 512 (32 x 32 feature pixels each: 8192 rows per domain),
input_nc = 2048, ndf = 512, num_classes = 6: HIP-event time of every kernel of csrc/fada_kernels.hip and of the generic
routes on the discriminator's geometry, next to the alternative route for the head --
    head forward + loss:  rgda_fada_head (one MFMA tile per workgroup, soft labels / log-softmax / dz in its epilogue)
                          against rgda_conv2d with 32 output columns, alone and followed by an in-place elementwise pass over
                          the 32-column rows (the least a separate loss pass would cost: it would read the logits as well)
-- the arms alternating over ROUNDS rounds in one process; the median and the spread (min .. max) are printed.  The head's
data gradient has no generic arm: rgda_conv2d refuses an operand of 32 channels.  Then a SourceStep (the benchmark's model
and batch) without and with the term, alternating.
    python scripts/dev/fada_bench.py [calls] [--no-step]
TFLOP/s: 2 * rows * 9 * Cin * Cout per layer and pass over the time."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402
from regda_amd.models.PixelDiscriminator import PixelDiscriminator, backward_rows, trunk_rows  # noqa: E402

ROUNDS = 5
B, SIZE, NC_IN, NDF, C = 8, 512, 2048, 512, 6
BF = torch.bfloat16


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # us


def race(title, arms, calls, flops=None):
    """arms: [(name, fn)]; alternating rounds; prints median (min .. max) and returns the medians"""
    for _, fn in arms:
        for _ in range(2):
            fn()
    times = {n: [] for n, _ in arms}
    for _ in range(ROUNDS):
        for n, fn in arms:
            times[n].append(timed(fn, calls))
    med = {}
    for n, _ in arms:
        t = times[n]
        med[n] = statistics.median(t)
        rate = '  %6.1f TFLOP/s' % (flops / med[n] / 1e6) if flops else ''
        print('  %-30s %-52s %9.1f us (%.1f .. %.1f)%s' % (title, n, med[n], min(t), max(t), rate), flush=True)
    return med


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    calls = int(args[0]) if args else 20
    torch.manual_seed(0)
    d = PixelDiscriminator(NC_IN, NDF, C).cuda()
    op = d.operands()
    h = SIZE // 16
    M = B * h * h
    feat = torch.randn(B, NC_IN, h, h, device='cuda')
    logits = torch.randn(B, C, h, h, device='cuda') * 2
    X = ops.feat_pack_rows(feat)
    acts = trunk_rows(op, X, B, h, h)
    a1, a2 = acts[1], acts[2]
    loss = torch.zeros(1, device='cuda')
    dz = ops.fada_loss(a2, op.wf[2], op.bias[2], logits, 0, loss=loss)[1]
    print('feature-adversarial path, %d rows, input_nc = %d, ndf = %d, C = %d; %d calls per round, %d rounds' % (
        M, NC_IN, NDF, C, calls, ROUNDS), flush=True)
    dfeat = torch.zeros_like(feat)
    race('pixel rows', [('rgda_feat_pack_rows', lambda: ops.feat_pack_rows(feat, out=X)),
                        ('rgda_feat_unpack_rows', lambda: ops.feat_unpack_rows(X, dfeat))], calls)
    for i, (x, y) in enumerate(((X, a1), (a1, a2))):
        raw = torch.empty_like(y)
        flops = 2.0 * M * 9 * x.shape[1] * y.shape[1]
        wf, bias = op.wf[i], op.bias[i]

        def fwd():
            ops.conv2d(x, wf, raw, B, h, h, h, h, 3, 3, 1, 1, 1)
            ops.disc_bias_lrelu(raw, bias)
        race('D.%d forward %d -> %d' % (2 * i, x.shape[1], y.shape[1]), [('rgda_conv2d + rgda_disc_bias_lrelu', fwd)], calls, flops)
    # the head: the fused kernel against the generic route
    zrows = torch.empty((M, ops.FADA_CP), dtype=BF, device='cuda')
    flops = 2.0 * M * 9 * a2.shape[1] * ops.FADA_CP

    def generic_head():
        ops.conv2d(a2, op.wf[2], zrows, B, h, h, h, h, 3, 3, 1, 1, 1)

    def generic_head_pass():
        generic_head()
        ops.disc_bias_lrelu(zrows, op.bias[2])
    race('heads %d -> 32' % a2.shape[1],
         [('rgda_fada_head (z stored, the module path)', lambda: ops.fada_head(a2, op.wf[2], op.bias[2], B, h, h, C)),
          ('rgda_fada_head (fused loss and dz) + loss sum', lambda: ops.fada_loss(a2, op.wf[2], op.bias[2], logits, 0, loss=loss)),
          ('rgda_conv2d, 32 columns', generic_head),
          ('rgda_conv2d, 32 columns + an in-place pass', generic_head_pass)], calls, flops)
    race('heads data gradient', [('rgda_fada_head_bwd_data (mask fused)', lambda: ops.fada_head_backward_data(dz, op.wt[2], a2, B, h, h))],
         calls, flops)
    g2 = ops.fada_head_backward_data(dz, op.wt[2], a2, B, h, h)
    g1 = torch.empty_like(a1)

    def d2_bwd():
        ops.conv2d(g2, op.wt[1], g1, B, h, h, h, h, 3, 3, 1, 1, 1, mode=1)
        ops.lrelu_mask_rows(g1, a1)
    race('D.2 data gradient', [('rgda_conv2d mode 1', lambda: ops.conv2d(g2, op.wt[1], g1, B, h, h, h, h, 3, 3, 1, 1, 1, mode=1)),
                               ('rgda_conv2d mode 1 + rgda_lrelu_mask_rows', d2_bwd)], calls, 2.0 * M * 9 * NDF * (NDF // 2))
    d2_bwd()
    rows = torch.zeros_like(X)
    race('D.0 data gradient', [('rgda_conv2d mode 1', lambda: ops.conv2d(g1, op.wt[0], rows, B, h, h, h, h, 3, 3, 1, 1, 1, mode=1)),
                               ('rgda_conv2d mode 1, res = y (the add onto the rows)',
                                lambda: ops.conv2d(g1, op.wt[0], rows, B, h, h, h, h, 3, 3, 1, 1, 1, mode=1, res=rows))],
         calls, 2.0 * M * 9 * NC_IN * NDF)
    for name, x, g in (('heads', a2, dz), ('D.2', a1, g2), ('D.0', X, g1)):
        dw = torch.zeros((g.shape[1], 9, x.shape[1]), dtype=torch.float32, device='cuda')

        def params():
            ops.conv2d_wgrad_grouped([(x, g, dw, B, h, h, h, h, 3, 3, 1, 1, 1)])
            ops.disc_bias_grad(g)
        race('%s parameters' % name, [('rgda_conv2d_wgrad_grouped + rgda_disc_bias_grad', params)], calls,
             2.0 * M * 9 * x.shape[1] * g.shape[1])

    def gen_pass():
        aa = trunk_rows(op, ops.feat_pack_rows(feat), B, h, h)
        gz = ops.fada_loss(aa[2], op.wf[2], op.bias[2], logits, 0, loss=loss)[1]
        backward_rows(op, gz, aa, B, h, h, need_dparams=False, onto=rows)

    def disc_pass():
        aa = trunk_rows(op, ops.feat_pack_rows(feat), B, h, h)
        gz = ops.fada_loss(aa[2], op.wf[2], op.bias[2], logits, 1, loss=loss)[1]
        backward_rows(op, gz, aa, B, h, h, need_dparams=True, need_dinput=False)

    race('one domain, 8 images', [('forward + input gradient (generator term)', gen_pass),
                                  ('forward + parameter gradients (one domain)', disc_pass)], max(calls // 4, 3))
    if '--no-step' in sys.argv:
        return
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.source import SourceStep
    from regda_amd.synthetic import make_batch
    torch.manual_seed(2333)
    model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False), multi_layer=True,
                           cascade=False, use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048,
                           num_classes=6, is_ins_norm=True))
    model.sync_weights()
    batch = make_batch(b=B, size=SIZE, seed=2333)
    arms = [('align_domain, without the term', SourceStep(model, align_domain=True)),
            ('align_domain, fada_weight = 0.001', SourceStep(model, align_domain=True, fada_weight=0.001))]

    def run(st):
        return lambda: st.step(batch['images_s'], batch['label_s'], batch['images_t'], 1e-3)

    m = race('SourceStep, resnet101', [(n, run(st)) for n, st in arms], 5)
    print('  the term costs %.2f ms per step' % ((m[arms[1][0]] - m[arms[0][0]]) / 1e3))


if __name__ == '__main__':
    main()
