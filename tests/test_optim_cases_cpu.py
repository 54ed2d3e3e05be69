"""CPU: the case tables of tests/optim_cases.py reach every path they name, every case is a call its entry point accepts,
the restated grid arithmetic still matches optim_kernels.hip, and the references are what they claim: the fp64 SGD step
equals torch.optim.SGD with clip_grad_norm_ in fp64, the integer bf16 rounding equals torch's, the rank-order cases depend
on the order, and the SplitMix64 mask keeps 1 - p of its elements and is a prefix of every longer one."""
import math
import os
import re

import numpy as np
import torch

import optim_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'optim_kernels.hip')).read()
COMMON = open(os.path.join(ROOT, 'regda_amd', 'csrc', 'common.h')).read()
HDR = open(os.path.join(ROOT, 'include', 'rgda_hip.h')).read()


def test_every_named_path_is_reached():
    reached = O.paths_reached()
    print('\n'.join('%-28s %s' % (p, ', '.join(sorted(set(reached.get(p, []))))[:150]) for p in O.REQUIRED))
    missing = [p for p in O.REQUIRED if not reached.get(p)]
    assert not missing, missing
    # and every case reaches what it claims to be there for
    for c in O.SGD_CASES:
        got = {p for p, names in reached.items() if c.name in names}
        assert set(c.paths) <= got, (c.name, set(c.paths) - got)
        want = {'active': 'sgd_clip_active', 'inactive': 'sgd_clip_inactive', 'zero': 'sgd_zero_grad',
                'tiny': 'sgd_tiny_norm'}[c.clip]
        assert want in got, (c.name, want)
    for name, why in (('vec', False), ('fallback', True)):
        assert all(bool(O.layout_fallback_reasons(r)) == why for r in O.LAYOUT_TABLES[name]), name
    # the cap cases go round the grid-stride loop more than once, the others named `stride` too
    assert O.loops(max(O.SUMSQ_N) >> 2, O.THREADS, O.sumsq_blocks(max(O.SUMSQ_N)))
    assert O.loops(max(c.n for c in O.SGD_CASES) >> 2, O.THREADS, O.SGD_CAP)
    assert O.loops(max(O.CAST_N) >> 2, O.THREADS, O.CAST_CAP) and O.loops(max(O.CASTF32_N), O.THREADS, O.CASTF32_CAP)
    assert O.loops(max(O.FILL_BYTES) >> 4, O.THREADS, O.FILL_CAP) and O.loops(O.COPY_BIG >> 4, O.THREADS, O.COPY_CAP)
    assert O.loops(max(s for _, s, _ in O.DDP_CASES) >> 3, O.THREADS, O.DDP_CAP)
    M, C, _ = O.ADD_CASES[-1]
    assert O.loops(M * C // 8, O.THREADS, O.ADD_CAP)


def test_cases_are_valid_calls():
    assert all(n > 0 for n in O.SUMSQ_N + O.CAST_N + O.CASTF32_N)
    for c in O.SGD_CASES:
        assert c.n > 0 and c.n % 4 == 0 and 0 <= c.ema < 1 and c.max_norm > 1e-6 and c.bufs in ('all', 'noshadow', 'nosb', 'nopb')
        assert math.log2(c.gscale) == int(math.log2(c.gscale))      # coef_fp32: the product by gscale is exact
    for w, s, order in O.DDP_CASES:
        assert w >= 1 and s > 0 and s % 8 == 0 and (not order or w >= 3)
    for name, rows in O.LAYOUT_TABLES.items():
        first, total = O.layout_first_blocks(rows)
        assert 0 < total < 2 ** 31 and first == sorted(first)
        for r in rows:
            assert min(r.Co, r.T, r.Ci) >= 1 and r.off + r.Ci <= r.ld and r.mode in (0, 1, 2) and 0 <= r.dst_off < 8
            assert math.prod(O.layout_dst_shape(r)) == r.Co * r.T * r.Ci
    assert all(r.Co == r.Ci == 4 and r.T == 1 for r in O.LAYOUT_TABLES['rows1025'])
    assert len(O.LAYOUT_TABLES['rows1025']) == 1025
    for R, K, Kp in O.PAD_CASES:
        assert R > 0 and 0 < K <= Kp
    assert (64, 147, 192) in O.PAD_CASES and any(K == Kp for _, K, Kp in O.PAD_CASES)
    for sizes in O.COPY_CASES:
        assert 1 <= len(sizes) <= O.COPY_MAX_JOBS and all(b % 16 == 0 for b in sizes)
    for p, s, n in O.DROPOUT_CASES:
        assert 0 <= p < 1 and 0 <= s < 2 ** 64 and n > 0
    assert {(p, s) for p, s, _ in O.DROPOUT_CASES} >= {(p, s) for p in O.DROPOUT_P for s in O.DROPOUT_SEEDS}
    for M, C, lds in O.ADD_CASES:
        assert M > 0 and C % 8 == 0 and all(ld % 8 == 0 and ld >= C for ld in lds)
    assert len({lds for *_, lds in O.ADD_CASES}) >= 3


def _ints(pattern, src=SRC):
    m = re.search(pattern, src)
    assert m, pattern
    return tuple(int(x) for x in m.groups())


def test_restatement_matches_the_source():
    assert _ints(r'#define\s+RGDA_LAYOUT_TILE\s+(\d+)', HDR) == (O.LAYOUT_TILE,)
    assert re.search(r'static inline int cdiv\(long long a, long long b\) \{ return \(int\)\(\(a \+ b - 1\) / b\); \}', COMMON)
    assert _ints(r'rgda_sumsq\(.*?int blocks = min\(cdiv\(n, (\d+) \* (\d+)\), (\d+)\);', re.sub(r'\n', ' ', SRC)) == \
        (256, 16, O.SUMSQ_CAP) and O.SUMSQ_PER_BLOCK == 256 * 16
    assert _ints(r'int blocks = min\(cdiv\(n4, (\d+) \* (\d+)\), (\d+)\);') == (256, 4, O.SGD_CAP)
    assert O.SGD_VEC_PER_BLOCK == 256 * 4 and re.search(r'long long n4 = n >> 2;\s*int blocks = min\(cdiv\(n4,', SRC)
    assert re.search(r'n <= 0 \|\| \(n & 3\)\) return RGDA_ERR_ARG', SRC)
    flat = re.sub(r'\s+', ' ', SRC)
    assert _ints(r'rgda_cast_bf16\(.*?int blocks = min\(cdiv\(n, (\d+) \* (\d+)\), (\d+)\);', flat) == (256, 16, O.CAST_CAP)
    assert _ints(r'cast_f32_kernel<<<min\(cdiv\(n, (\d+) \* (\d+)\), (\d+)\), 256,', flat) == (256, 8, O.CASTF32_CAP)
    assert _ints(r'const int blocks = min\(cdiv\(shard_elems >> 3, (\d+)\), (\d+)\);') == (O.THREADS, O.DDP_CAP)
    assert re.search(r'\(shard_elems & 7\)\) return RGDA_ERR_ARG', SRC)
    assert _ints(r'fill_zero_kernel<<<\(int\)min\(\(long long\)cdiv\(n16 > 0 \? n16 : 1, (\d+) \* (\d+)\), (\d+)ll\), 256,',
                 flat) == (256, 4, O.FILL_CAP)
    assert _ints(r'blocks \+= \(int\)min\(\(long long\)cdiv\(j\.n16\[k\] > 0 \? j\.n16\[k\] : 1, (\d+) \* (\d+)\), (\d+)ll\);') == \
        (256, 4, O.COPY_CAP)
    assert re.search(r'j\.first\[k\] = blocks;', SRC) and re.search(r'for \(int k = n; k <= 4; \+\+k\) j\.first\[k\] = blocks;', SRC)
    assert _ints(r'if \(n < 1 \|\| n > (\d+) \|\|') == (O.COPY_MAX_JOBS,)
    assert _ints(r'dropout_mask_kernel<<<min\(cdiv\(n, (\d+)\), (\d+)\), 256,') == (O.THREADS, O.DROPOUT_CAP)
    assert _ints(r'add_bf16_kernel<<<min\(cdiv\(total, (\d+)\), (\d+)\), 256,') == (O.THREADS, O.ADD_CAP)
    assert re.search(r'long long total = M \* \(C / 8\);', SRC)
    assert re.search(r'pad_cast_kernel<<<cdiv\(\(long long\)R \* Kp, 256\), 256,', SRC)
    assert re.search(r'unpad_acc_kernel<<<cdiv\(\(long long\)R \* K, 256\), 256,', SRC)
    # the layout kernel: the tile, the blocks of a row, the LDS row limit, the vectorised-path predicate
    assert re.search(r'constexpr int TS = RGDA_LAYOUT_TILE;', SRC)
    assert re.search(r'const int nci = \(Ci \+ TS - 1\) / TS, nco = \(Co \+ TS - 1\) / TS;', SRC)
    assert re.search(r'const int bx = rel % nci; rel /= nci;\s*const int by = rel % nco;\s*const int tap = rel / nco;', SRC)
    assert _ints(r'constexpr int NFB = (\d+);') == (O.LAYOUT_LDS_ROWS,)
    assert re.search(r'const bool src16 = \(\(int\)e\[7\] & (\d+)\) != 0;', SRC).group(1) == str(O.LAYOUT_SRC16)
    assert ('const bool vec = !(Ci & 3) && !(sld & 3) && !((size_t)w & (src16 ? 7 : 15)) && !((size_t)wt & 7) && '
            '(mode != 0 || !(Co & 3));') in SRC
    # the dropout generator's constants
    for c in (O._GOLDEN, O._M1, O._M2):
        assert '0x%Xull' % c in SRC
    assert 'const float u = (float)(z >> 40) * 0x1p-24f;' in SRC and '(unsigned long long)(i + 1)' in SRC


def test_grid_arithmetic_examples():
    assert O.copy_first([16]) == [0, 1, 1, 1, 1]
    assert O.copy_first([16 * 1025, 16, 16 * 4097, 16 * 3]) == [0, 2, 3, 8, 9]
    assert O.copy_first([O.COPY_BIG, 16]) == [0, 2048, 2049, 2049, 2049]
    assert O.copy_first([16, 0, 32]) == [0, 1, 2, 3, 3]
    assert O.fill_blocks(0) == 1 and O.fill_blocks(15) == 1 and O.fill_blocks(max(O.FILL_BYTES)) == 4096
    assert O.layout_blocks(130, 65, 9) == 3 * 2 * 9 and O.layout_blocks(4, 4, 1) == 1
    assert O.sgd_blocks(4) == 1 and O.sgd_blocks(O.RAGGED) == 3 and O.sgd_blocks(max(c.n for c in O.SGD_CASES)) == 4096
    assert O.sumsq_blocks(4 * O.K + 1) == 2 and O.sumsq_blocks(max(O.SUMSQ_N)) == 1024
    assert O.pad_blocks(64, 147, 192) == (48, 37)


def test_sgd_reference_is_torch_sgd_with_clip_grad_norm_in_fp64():
    """Three steps of every hyper-parameter set of the table, in fp64 throughout (coef formed in fp64 as well): the
    reference written from the definitions against torch's own optimizer and clipping."""
    hyper = sorted({(c.gscale, c.wd, c.ema, c.max_norm, c.gsig) for c in O.SGD_CASES})
    gen = torch.Generator().manual_seed(5)
    n = 64
    for gscale, wd, ema, max_norm, gsig in hyper:
        p0 = torch.randn(n, generator=gen, dtype=torch.float64)
        par = torch.nn.Parameter(p0.clone())
        opt = torch.optim.SGD([par], lr=O.SGD_LR, momentum=O.SGD_MOMENTUM, weight_decay=wd)
        p, v, s = p0.clone(), torch.full((n,), float('nan'), dtype=torch.float64), p0.clone()
        s_t = p0.clone()
        for step in range(3):
            g = torch.randn(n, generator=gen, dtype=torch.float64) * gsig * (n / 1024) ** -0.5
            par.grad = g * gscale                        # the gradient averaged over the ranks
            total_t = torch.nn.utils.clip_grad_norm_([par], max_norm)
            opt.step()
            s_t = (1 - ema) * par.detach() + ema * s_t
            total = float((g * g).sum().sqrt()) * gscale
            assert total == float(total_t) or abs(total - float(total_t)) < 1e-12 * total
            coef = min(max_norm / (total + 1e-6), 1.0) * gscale
            v, p, s, *_ = O.sgd_reference(p, g, v, s, coef, 0.0, O.SGD_LR, O.SGD_MOMENTUM, wd, ema, step == 0)
            key = (gscale, wd, ema, max_norm, gsig, step)
            torch.testing.assert_close(p, par.detach(), rtol=1e-13, atol=1e-15, msg=str(key))
            torch.testing.assert_close(s, s_t, rtol=1e-13, atol=1e-15, msg=str(key))
            buf = opt.state[par]['momentum_buffer']
            torch.testing.assert_close(v, buf, rtol=1e-13, atol=1e-15, msg=str(key))
        assert not torch.equal(p, p0) or gsig == 0 and wd == 0


def test_coef_fp32_against_fp64():
    for gn, gscale, max_norm in ((4.0e-10, 1.0, 1e-5), (9216.0, 0.5, 1.0), (0.0, 1.0, 32.0), (1.0, 0.125, 1e4),
                                 (3.7e7, 0.5, 32.0)):
        coef, rel = O.coef_fp32(gn, gscale, max_norm)
        total = math.sqrt(float(np.float32(gn))) * gscale
        ref = min(float(np.float32(max_norm)) / (total + float(np.float32(1e-6))), 1.0) * gscale
        assert abs(coef - ref) <= 4 * O.U32 * ref, (gn, coef, ref)
        assert (rel == 0.0) == (ref == gscale)
    # the tiny-norm case: the 1e-6 moves coef by percents
    coef, _ = O.coef_fp32(4.0e-10, 1.0, 1e-5)
    assert abs(coef / (1e-5 / 2e-5) - 1) > 0.04


def test_bf16_rounding_in_integers_is_torch_rounding():
    gen = torch.Generator().manual_seed(2)
    x = torch.cat([torch.randn(4096, generator=gen), torch.randn(4096, generator=gen) * 1e-30,
                   torch.randn(4096, generator=gen) * 1e30, O.cast_specials()])
    got = O.bf16_bits(x)
    assert torch.equal(got, O.bf16_canon(x.to(torch.bfloat16)))
    sp = dict(zip(O.CAST_SPECIALS_BITS, O.bf16_bits(O.cast_specials()).tolist()))
    assert sp[0x3F808000] == 0x3F80 and sp[0x3F818000] == 0x3F82 and sp[0xBF808000] == 0xBF80 and sp[0xBF818000] == 0xBF82
    assert sp[0x7F7FFFFF] == 0x7F80 and sp[0xFF7FFFFF] == 0xFF80 and sp[0x7F7F7FFF] == 0x7F7F
    assert sp[0x7FC00000] == sp[0xFFC00001] == sp[0x7F800001] == O.BF16_NAN and sp[0x80000000] == 0x8000
    assert torch.equal(O.bf16_canon(O.bf16_from_bits(got)), got)


def test_rank_order_cases_depend_on_the_order():
    a, b, c = O.ORDER_TRIPLE
    f = np.float32
    assert f(f(f(a) + f(b)) + f(c)) == f(c) and f(f(f(c) + f(b)) + f(a)) == 0
    assert all(float(torch.tensor(v).to(torch.bfloat16)) == v for v in O.ORDER_TRIPLE)
    for world, s, order in O.DDP_CASES:
        if not order:
            continue
        recv = O.ddp_input(world, s, order, 'cpu')
        fwd, rev = O.ddp_reference_bits(recv, world), O.ddp_reference_bits(recv, world, descending=True)
        assert not torch.equal(fwd, rev), (world, s)


def test_dropout_reference_keep_fraction_and_prefix():
    # the first outputs of SplitMix64 seeded with 0 (the published test vector of the generator)
    assert [int(z) for z in O.splitmix64(0, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for p, seed, n in O.DROPOUT_CASES:
        m = O.dropout_reference(n, p, seed)
        keep = np.float32(1) / (np.float32(1) - np.float32(p))
        assert set(np.unique(m).tolist()) <= {0.0, float(keep)}
        q = 1.0 - float(np.float32(p))
        assert abs((m != 0).sum() - n * q) <= 4 * math.sqrt(n * q * (1 - q)), (p, seed, n)
    for p in O.DROPOUT_P:
        for seed in O.DROPOUT_SEEDS:
            n1, n2 = 1000, 4099
            assert np.array_equal(O.dropout_reference(n1, p, seed), O.dropout_reference(n2, p, seed)[:n1])
    assert not np.array_equal(O.dropout_reference(4099, 0.5, 0), O.dropout_reference(4099, 0.5, 2 ** 62 - 1))
