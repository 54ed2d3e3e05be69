"""The adversarial path at b = 8, 512 x 512, ndf = 64, C = 6: HIP-event time of every kernel of csrc/adv_kernels.hip and of
the generic weight gradient on the discriminator's geometry, next to the parent's routes for the same work --
    data gradient of layers 2-4:  rgda_disc_conv_bwd_data (four parity sub-convolutions, LeakyReLU mask fused) against
                                  rgda_conv2d mode 1, alone and followed by an in-place elementwise pass (the least a
                                  separate mask pass would cost)
    forward of layers 2-4:        rgda_disc_conv_fwd (bias + LeakyReLU in the epilogue) against rgda_conv2d + the separate
                                  bias / LeakyReLU pass rgda_disc_bias_lrelu (the route FCDiscriminator takes)
-- the arms alternating over ROUNDS rounds in one process; the median and the spread (min .. max) are printed.  Then an
AlignStep (the benchmark's model and batch) without and with the term, alternating.
    python scripts/dev/adv_bench.py [calls] [--no-step]
TFLOP/s: 2 * pixels_out * 16 * Cin * Cout per layer and pass (the useful operations, the padding channels of the first
layer included) over the time."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from regda_amd import ops  # noqa: E402
from regda_amd.models.Discriminator import FCDiscriminator, backward_rows, forward_rows  # noqa: E402

ROUNDS = 5
B, SIZE, NDF, C = 8, 512, 64, 6
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
        print('  %-34s %-44s %9.1f us (%.1f .. %.1f)%s' % (title, n, med[n], min(t), max(t), rate))
    return med


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    calls = int(args[0]) if args else 20
    torch.manual_seed(0)
    d = FCDiscriminator(C, ndf=NDF).cuda()
    op = d.operands()
    logits = (torch.randn(B, C, SIZE // 16, SIZE // 16) * 2).cuda()
    glog = torch.zeros_like(logits)
    size = (SIZE, SIZE)
    P = ops.adv_probs(logits, size)
    z, acts = forward_rows(op, P, B, SIZE, SIZE)
    _, dz = ops.bce_logits(z, 0.0)
    print('adversarial path, b = %d, %d x %d, ndf = %d, C = %d; %d calls per round, %d rounds' % (B, SIZE, SIZE, NDF, C, calls, ROUNDS))
    dP = torch.randn(P.shape, device='cuda').to(BF)
    race('probabilities', [('rgda_adv_probs_fwd', lambda: ops.adv_probs(logits, size, out=P)),
                           ('rgda_adv_probs_bwd', lambda: ops.adv_probs_backward(dP, logits, glog, size))], calls)
    h = SIZE
    for i in range(4):
        x, y = acts[i], acts[i + 1]
        Cin, Cout = x.shape[1], y.shape[1]
        g = torch.randn(y.shape, device='cuda').to(BF)
        flops = 2.0 * y.shape[0] * 16 * Cin * Cout
        wf, wt, bias = op.wf[i], op.wt[i], op.bias[i]
        hh = h
        fwd = [('rgda_disc_conv_fwd', lambda: ops.disc_conv(x, wf, bias, B, hh, hh, out=y))]
        bwd = [('rgda_disc_conv_bwd_data (parity)', lambda: ops.disc_conv_backward(g, x, wt, B, hh, hh, below=i > 0, need_dparams=False))]
        if Cin % 64 == 0:
            raw, dx = torch.empty_like(y), torch.empty_like(x)

            def generic():
                ops.conv2d(x, wf, raw, B, hh, hh, hh // 2, hh // 2, 4, 4, 2, 1, 1)

            def generic_epilogue():
                generic()
                ops.disc_bias_lrelu(raw, bias)

            fwd += [('rgda_conv2d', generic), ('rgda_conv2d + rgda_disc_bias_lrelu', generic_epilogue)]
            zero = torch.zeros(Cin, device='cuda')

            def generic_bwd():
                ops.conv2d(g, wt, dx, B, hh // 2, hh // 2, hh, hh, 4, 4, 2, 1, 1, mode=1)

            def generic_bwd_pass():       # + an in-place elementwise pass over dx: the LEAST a separate mask pass costs (it
                generic_bwd()             # would read the activation as well)
                ops.disc_bias_lrelu(dx, zero)

            bwd += [('rgda_conv2d mode 1 (no mask)', generic_bwd), ('rgda_conv2d mode 1 + an in-place pass', generic_bwd_pass)]
        race('layer %d forward %d -> %d' % (i + 1, Cin, Cout), fwd, calls, flops)
        race('layer %d data gradient' % (i + 1), bwd, calls, flops)
        race('layer %d parameters' % (i + 1),
             [('rgda_conv2d_wgrad_grouped + bias sums', lambda: ops.disc_conv_backward(g, x, wt, B, hh, hh, need_dx=False))], calls, flops)
        h //= 2
    race('head', [('rgda_disc_head_fwd', lambda: ops.disc_head(acts[4], op.wh, op.bh, B, h, h)),
                  ('rgda_disc_head_bwd', lambda: ops.disc_head_backward(dz, acts[4], op.wh, B, h, h)),
                  ('rgda_bce_logits', lambda: ops.bce_logits(z, 1.0))], calls)

    def gen_pass():
        zz, aa = forward_rows(op, ops.adv_probs(logits, size), B, SIZE, SIZE)
        g0 = backward_rows(op, ops.bce_logits(zz, 0.0)[1], aa, B, SIZE, SIZE, need_dparams=False)[0]
        ops.adv_probs_backward(g0, logits, glog, size)

    def disc_pass():
        zz, aa = forward_rows(op, ops.adv_probs(logits, size), B, SIZE, SIZE)
        backward_rows(op, ops.bce_logits(zz, 1.0)[1], aa, B, SIZE, SIZE, need_dparams=True, need_dinput=False)

    race('one head, 8 images', [('forward + input gradient (generator term)', gen_pass),
                                ('forward + parameter gradients (one domain)', disc_pass)], max(calls // 4, 3))
    if '--no-step' in sys.argv:
        return
    from regda_amd.align import AlignStep
    from regda_amd.models.Encoder import Deeplabv2
    from regda_amd.synthetic import make_batch
    torch.manual_seed(2333)
    model = Deeplabv2(dict(backbone=dict(resnet_type='resnet101', output_stride=16, pretrained=False), multi_layer=True,
                           cascade=False, use_ppm=True, ppm=dict(num_classes=6, use_aux=False, fc_dim=2048), inchannels=2048,
                           num_classes=6, is_ins_norm=True))
    with torch.no_grad():
        for head in ('layer5', 'layer6'):
            model.convs[f'{head}.conv_last.4'].w.mul_(40.0)
    model.sync_weights()
    protos = torch.randn(6, 2048, generator=torch.Generator().manual_seed(0))
    batch = make_batch(b=B, size=SIZE, seed=2333)
    plain = AlignStep(model, protos)
    adv = AlignStep(model, protos, adv_weight=0.001)

    def run(st):
        return lambda: st.step(batch['images_s'], batch['label_s'], batch['images_t'], batch['regs_t'], 1e-3)

    m = race('AlignStep, resnet101', [('without the term', run(plain)), ('adv_weight = 0.001, two heads', run(adv))], 5)
    print('  the term costs %.2f ms per step' % ((m['adv_weight = 0.001, two heads'] - m['without the term']) / 1e3))


if __name__ == '__main__':
    main()
