"""GPU: rgda_domain_mix_table, rgda_mix_select_classes and rgda_mix_write_table per element.  The table mix against
tests/mix_ref.py applied image by image with that image's row, the select against tests/mix_select_ref.py.  The kernels
copy and OR, nothing rounds: every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import mix_ref
import mix_select_ref
from mix_ref import bits_equal

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def make(n, c, h, w, seed, bad=None):
    """-> numpy source image / label (with -1, every class somewhere when the tile has room), clean image, label, soft"""
    rng = np.random.default_rng(seed)
    img_s = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    img_t = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    lab_s = rng.integers(-1, c, size=(n, h, w)).astype(np.int64)
    if bad is not None:
        lab_s[bad] = c + 3
    lab_t = rng.integers(-1, c, size=(n, h, w)).astype(np.int64)
    soft = rng.random((n, c, h, w)).astype(np.float32)
    return img_s, lab_s, img_t, lab_t, soft


def unaligned(a):
    """`a` on the device as a contiguous view whose first byte is NOT on a 16-byte boundary"""
    t = torch.from_numpy(a)
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def dev(a, misalign=False):
    return unaligned(a) if misalign else torch.from_numpy(a).to(DEV)


def table_of(rows):
    return torch.tensor(rows, dtype=torch.int64).to(torch.int32).to(DEV).contiguous()


def expect(img_s, lab_s, img_t, lab_t, soft, c, preds):
    """mix_ref image by image with that image's predicate -> (img, lab, soft, flag)"""
    outs, flag = [], 0
    for i, pred in enumerate(preds):
        s = slice(i, i + 1)
        img, lab, sf, _, f, _ = mix_ref.domain_mix(img_s[s], lab_s[s], img_t[s], label_t=lab_t[s], soft_t=soft[s], C=c, **pred)
        outs.append((img, lab, sf))
        flag |= f
    return [np.concatenate([o[k] for o in outs]) for k in range(3)] + [flag]


def run_cases(n, c, h, w, mode, rows, preds, misalign=False, bad=None, with_soft=None):
    from regda_amd import ops
    img_s, lab_s, img_t, lab_t, soft = make(n, c, h, w, seed=100 * c + h + w, bad=bad)
    want_img, want_lab, want_soft, want_flag = expect(img_s, lab_s, img_t, lab_t, soft, c, preds)
    table = table_of(rows)
    d = lambda a: dev(a, misalign)
    g_img_s, g_lab_s, g_in = d(img_s), d(lab_s), d(img_t)
    # images only
    out = d(np.full_like(img_t, np.nan))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.domain_mix_table(g_img_s, g_lab_s, table, mode, images_in=g_in, images_out=out, class_num=c, flag=flag)
    assert bits_equal(out.cpu().numpy(), want_img), 'image, out of place'
    assert bits_equal(g_in.cpu().numpy(), img_t), 'img_in was written'
    assert int(flag.item()) == want_flag
    # labels only (null images)
    g_lab = d(lab_t)
    flag.zero_()
    ops.domain_mix_table(g_img_s, g_lab_s, table, mode, label_t=g_lab, class_num=c, flag=flag)
    assert bits_equal(g_lab.cpu().numpy(), want_lab), 'label, null images'
    assert int(flag.item()) == want_flag
    # everything at once: the image, labels and soft planes
    if with_soft if with_soft is not None else c == 16:
        out2, g_lab2, g_soft = d(np.zeros_like(img_t)), d(lab_t), d(soft)
        ops.domain_mix_table(g_img_s, g_lab_s, table, mode, images_in=g_in, images_out=out2, label_t=g_lab2, soft_t=g_soft)
        assert bits_equal(out2.cpu().numpy(), want_img) and bits_equal(g_lab2.cpu().numpy(), want_lab)
        assert bits_equal(g_soft.cpu().numpy(), want_soft), 'soft planes'
        g_lab3, g_soft3 = d(lab_t), d(soft)
        ops.domain_mix_table(g_img_s, g_lab_s, table, mode, label_t=g_lab3, soft_t=g_soft3)
        assert bits_equal(g_lab3.cpu().numpy(), want_lab) and bits_equal(g_soft3.cpu().numpy(), want_soft)
        assert bits_equal(g_in.cpu().numpy(), img_t)
    # the sources are read only
    assert bits_equal(g_img_s.cpu().numpy(), img_s) and bits_equal(g_lab_s.cpu().numpy(), lab_s)
    return want_img, img_t


@pytest.mark.parametrize('hw', [(3, 5), (8, 8), (4, 12), (64, 64)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('c', [6, 7, 16])
def test_table_class_mode_per_image_class_sets(c, hw):
    """Image 0: no class, image 1: every class, image 2: a subset of its own; labels include -1."""
    from regda_amd import ops
    h, w = hw
    subset = [1, c - 1] if c < 16 else [0, 3, 9, 15]
    bits = [0, (1 << c) - 1, ops.mix_class_bits(subset, c)]
    rows = [[b, 0, 0, 0, 0, 0, 0, 0] for b in bits]
    preds = [dict(classes=[]), dict(classes=list(range(c))), dict(classes=subset)]
    mixed, clean = run_cases(3, c, h, w, ops.MIX_CLASS, rows, preds)
    assert bits_equal(mixed[0], clean[0]) and (h * w < 64 or not bits_equal(mixed[2], clean[2]))
    if hw == (4, 12):      # no pointer 16-byte aligned: the element route
        run_cases(3, c, h, w, ops.MIX_CLASS, rows, preds, misalign=True)


def test_table_class_mode_flag_follows_the_images_own_row():
    """A label that is neither a class nor -1 raises the flag only in an image whose class set is not empty."""
    from regda_amd import ops
    c = 6
    rows = [[0, 0, 0, 0, 0, 0, 0, 0], [0b1010, 0, 0, 0, 0, 0, 0, 0]]
    preds = [dict(classes=[]), dict(classes=[1, 3])]
    run_cases(2, c, 4, 8, ops.MIX_CLASS, rows, preds, bad=(0, 1, 2))        # in the image that reads no label: no flag
    run_cases(2, c, 4, 8, ops.MIX_CLASS, rows, preds, bad=(1, 3, 7))        # in the other one: flag
    run_cases(2, c, 3, 5, ops.MIX_CLASS, rows, preds, bad=(1, 2, 4))        # at the ragged row end


@pytest.mark.parametrize('hw', [(8, 8), (5, 7)], ids=lambda s: '%dx%d' % s)
def test_table_box_mode_per_image_boxes(hw):
    """Empty, the full tile, a single pixel, and x0 = 3, x1 = 6, which straddles a quad; ignore labels are copied."""
    from regda_amd import ops
    h, w = hw
    boxes = [(2, 2, 1, 4), (0, h, 0, w), (h - 1, h, w - 1, w), (1, h - 1, 3, 6)]
    rows = [[0, *b, 0, 0, 0] for b in boxes]
    preds = [dict(box=b) for b in boxes]
    mixed, clean = run_cases(4, 6, h, w, ops.MIX_BOX, rows, preds, with_soft=True)
    assert bits_equal(mixed[0], clean[0])
    run_cases(4, 6, h, w, ops.MIX_BOX, rows, preds, with_soft=True, bad=(3, 2, 4))      # inside image 3's box: pasted, flag
    run_cases(4, 6, h, w, ops.MIX_BOX, rows, preds, with_soft=True, bad=(3, 0, 4))      # outside it: not read
    if hw == (8, 8):
        run_cases(4, 6, h, w, ops.MIX_BOX, rows, preds, with_soft=True, misalign=True)


def test_table_mix_in_place_and_wrapper_checks():
    from regda_amd import ops
    img_s, lab_s, img_t, lab_t, soft = make(2, 6, 8, 8, seed=3)
    rows = [[0b11, 0, 0, 0, 0, 0, 0, 0], [0b100, 0, 0, 0, 0, 0, 0, 0]]
    want = expect(img_s, lab_s, img_t, lab_t, soft, 6, [dict(classes=[0, 1]), dict(classes=[2])])[0]
    g = dev(img_t)
    ops.domain_mix_table(dev(img_s), dev(lab_s), table_of(rows), ops.MIX_CLASS, images_in=g, images_out=g, class_num=6)
    assert bits_equal(g.cpu().numpy(), want)         # img_out may be img_in
    t = table_of(rows)
    with pytest.raises(ValueError):
        ops.domain_mix_table(dev(img_s), dev(lab_s), t, ops.MIX_CLASS, images_in=g)
    with pytest.raises(ValueError):
        ops.domain_mix_table(dev(img_s), dev(lab_s), t.to(torch.int64), ops.MIX_CLASS, images_in=g, images_out=g)
    with pytest.raises(ValueError):
        ops.domain_mix_table(dev(img_s), dev(lab_s).int(), t, ops.MIX_CLASS, images_in=g, images_out=g)
    with pytest.raises(ValueError):
        ops.domain_mix_table(dev(img_s), dev(lab_s), t, ops.MIX_CLASS, label_t=dev(lab_t).transpose(1, 2))
    with pytest.raises(ValueError):
        ops.domain_mix_table(dev(img_s), dev(lab_s), t[:1], ops.MIX_CLASS, images_in=g, images_out=g)


# -------------------------------------------------------------------------------------------------------------- select
def select_case(lab, ranks, ws=None, misalign=False):
    """-> the table after the call (numpy), the flag, the workspace; column 0 against the numpy rule, the other columns
    and the words behind the table and the workspace untouched"""
    from regda_amd import ops
    n, c = ranks.shape
    big = torch.full((n + 2, 8), 77, dtype=torch.int32, device=DEV)
    table = big[:n]
    if ws is None:
        ws = torch.full((n + 4,), -1, dtype=torch.int32, device=DEV)       # stale bits everywhere: the call clears its N words
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.mix_select_classes(dev(lab, misalign), torch.from_numpy(ranks).to(DEV), table, ws=ws, flag=flag)
    got = big.cpu().numpy()
    want_bits, want_flag = mix_select_ref.select_classes(lab, ranks)
    assert got[:n, 0].view(np.uint32).tolist() == want_bits.tolist()
    assert (got[:n, 1:] == 77).all() and (got[n:] == 77).all(), 'written outside table[n][0]'
    assert (ws[n:].cpu().numpy() == -1).all() or ws.numel() == n, 'written behind the workspace'
    assert int(flag.item()) == want_flag
    return want_bits, ws


def perms(n, c, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(c) for _ in range(n)]).astype(np.uint8)


@pytest.mark.parametrize('hw', [(3, 5), (64, 64), (31, 33)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('c', [6, 16])
def test_select_matches_the_numpy_rule(c, hw):
    h, w = hw
    rng = np.random.default_rng(7 * c + h)
    lab = rng.integers(-1, c, size=(3, h, w)).astype(np.int64)
    lab[1] = rng.choice([-1, 0, c - 1], size=(h, w))                # three present classes at most
    lab[2] = -1                                                     # an image of ignore labels only
    bits, _ = select_case(lab, perms(3, c, seed=c + w))
    assert bits[2] == 0 and bits[0] != 0


def test_select_sees_a_class_that_occurs_only_at_the_last_pixel_of_a_ragged_row():
    for h, w in ((3, 5), (7, 9), (1, 1), (64, 63)):
        lab = np.zeros((2, h, w), np.int64)
        lab[0, -1, -1] = 4
        lab[1, 0, -1] = 5
        ranks = np.array([[5, 4, 3, 2, 0, 1], [1, 2, 3, 4, 5, 0]], np.uint8)       # the lone class ranks before class 0
        bits, _ = select_case(lab, ranks)
        assert bits.tolist() == [1 << 4, 1 << 5]
        select_case(lab[:, :, ::-1].copy(), ranks, misalign=(h * w) % 2 == 0)      # the element route on an even tile


def test_select_all_sixteen_classes_present_and_the_unmixed_batch():
    lab = np.arange(16, dtype=np.int64).repeat(4).reshape(1, 8, 8)
    ranks = perms(1, 16, seed=2)
    bits, _ = select_case(lab, ranks)
    assert bin(int(bits[0])).count('1') == 8
    assert select_case(lab, np.full((1, 16), 255, np.uint8))[0].tolist() == [0]


def test_select_reused_workspace_keeps_no_stale_presence_bits():
    ranks = np.array([[0, 1, 2, 3, 4, 5]] * 2, np.uint8)
    first = np.full((2, 8, 8), 5, np.int64)
    first[:, 0, :3] = [0, 1, 2]
    bits, ws = select_case(first, ranks)
    assert bits.tolist() == [0b11, 0b11]
    second = np.full((2, 8, 8), 5, np.int64)            # classes 0..2 are gone: a stale bit would keep class 0 selected
    bits, _ = select_case(second, ranks, ws=ws)
    assert bits.tolist() == [1 << 5, 1 << 5]


def test_select_out_of_range_label_sets_the_flag_and_is_skipped():
    lab = np.full((2, 6, 6), 1, np.int64)
    lab[0, 2, 3] = 40               # at or above 32: a shift by it would leave the word
    lab[1, 5, 5] = -7
    lab[1, 0, 0] = 6                # == C
    bits, _ = select_case(lab, perms(2, 6, seed=1))
    assert bits.tolist() == [1 << 1, 1 << 1]


# --------------------------------------------------------------------------------------------------------- write_table
def test_write_table_carries_the_draw_in_its_arguments():
    from regda_amd import ops
    n, c = 5, 7
    big = torch.full((n + 1, 8), 77, dtype=torch.int32, device=DEV)
    ops.mix_write_table(big[:n], c, class_bits=0b1000101)
    assert big.cpu().numpy().tolist() == mix_select_ref.table_rows(n, 0b1000101).tolist() + [[77] * 8]
    ops.mix_write_table(big[:n], c, box=(1, 9, 3, 6))
    assert big[:n].cpu().numpy().tolist() == mix_select_ref.table_rows(n, 0, (1, 9, 3, 6)).tolist()
    ranks_host = perms(n, c, seed=4)
    ranks = torch.full((n + 1, c), 9, dtype=torch.uint8, device=DEV)
    ops.mix_write_table(big[:n], c, ranks=ranks[:n], ranks_host=ranks_host)
    ranks_host_sent = ranks_host.copy()
    ranks_host[:] = 0               # the host buffer is free once the call has returned
    torch.cuda.synchronize()
    assert ranks[:n].cpu().numpy().tolist() == ranks_host_sent.tolist() and ranks[n].tolist() == [9] * c
    assert (big[:n].cpu().numpy() == 0).all()
    full = torch.zeros(16, 8, dtype=torch.int32, device=DEV)
    ops.mix_write_table(full, 32, class_bits=1 << 31, ranks=torch.zeros(16, 32, dtype=torch.uint8, device=DEV),
                        ranks_host=perms(16, 32, seed=5))
    assert full.cpu().numpy().tolist() == mix_select_ref.table_rows(16, 1 << 31).tolist()
    with pytest.raises(ValueError):         # RGDA_ERR_UNSUPPORTED: more images than the argument block holds
        ops.mix_write_table(torch.zeros(17, 8, dtype=torch.int32, device=DEV), 6)
