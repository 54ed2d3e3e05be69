"""Mint tests/golden/augment.npz from the reference's OWN transforms (regda/aug/augmentation.py), behind a torchvision
stub that restates the four functions it calls as torchvision states them (F.hflip / vflip / crop / normalize and
T.RandomCrop.get_params; torchvision is not installed here).

Run in the build container only (needs the reference checkout):  python tests/golden/make_augment_goldens.py
Data only: inputs and the reference's outputs.
  small: one seeded uint8 3 x 48 x 40 image converted as basedata.py:70-72 (`.float().permute(2, 0, 1)` of the HWC
         array), a 6 x 48 x 40 soft label and an int64 region map; per seed s (random.seed(s), torch.manual_seed(s))
         Compose([RandomCrop((32, 32)), RandomHorizontalFlip(0.5), RandomVerticalFlip(0.5), RandomRotate90(0.5),
         Normalize(MEAN, STD, clamp=True)]) -> image, mask (the soft label), mask_sup; the next draw of each generator
         after the transform (random.random(), torch.rand(1)), which pins how many draws were consumed; and the
         parameters (y0, x0, d) read off the same seed applied to a coordinate image.  Seeds are chosen so that all 8
         dihedral elements appear, each at least twice.
  full:  a 512 x 512 input with a 512 crop (no crop draw): the image output and the next draws, for one seed."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import aug_ref  # noqa: E402

REF = '/root/reference'
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def _install_torchvision_stub():
    F = types.ModuleType('torchvision.transforms.functional')
    F.hflip = lambda img: img.flip(-1)
    F.vflip = lambda img: img.flip(-2)
    F.crop = lambda img, top, left, height, width: img[..., top:top + height, left:left + width]

    def normalize(tensor, mean, std, inplace=False):
        if not inplace:
            tensor = tensor.clone()
        mean = torch.as_tensor(mean, dtype=tensor.dtype, device=tensor.device)
        std = torch.as_tensor(std, dtype=tensor.dtype, device=tensor.device)
        if mean.ndim == 1:
            mean = mean.view(-1, 1, 1)
        if std.ndim == 1:
            std = std.view(-1, 1, 1)
        return tensor.sub_(mean).div_(std)
    F.normalize = normalize

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            h, w = img.shape[-2:]
            th, tw = output_size
            if h < th or w < tw:
                raise ValueError('Required crop size is larger than input image size')
            if w == tw and h == th:
                return 0, 0, h, w
            i = torch.randint(0, h - th + 1, size=(1,)).item()
            j = torch.randint(0, w - tw + 1, size=(1,)).item()
            return i, j, th, tw
    T = types.ModuleType('torchvision.transforms')
    T.RandomCrop = RandomCrop
    T.functional = F
    tv = types.ModuleType('torchvision')
    tv.transforms = T
    sys.modules.update({'torchvision': tv, 'torchvision.transforms': T, 'torchvision.transforms.functional': F})


def _load_reference():
    _install_torchvision_stub()
    spec = importlib.util.spec_from_file_location('ref_augmentation', os.path.join(REF, 'regda', 'aug', 'augmentation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pipeline(A, size, norm=True):
    ts = [A.RandomCrop(size), A.RandomHorizontalFlip(0.5), A.RandomVerticalFlip(0.5), A.RandomRotate90(0.5)]
    if norm:
        ts.append(A.Normalize(mean=MEAN, std=STD, clamp=True))
    return A.Compose(ts)


def _run(A, seed, size, image, mask=None, mask_sup=None, norm=True):
    random.seed(seed)
    torch.manual_seed(seed)
    blob = _pipeline(A, size, norm)(image=image, mask=mask, mask_sup=mask_sup)
    nxt = (random.random(), torch.rand(1).item())
    return blob, nxt


def _decode(A, seed, h, w, size):
    """(y0, x0, d) of one seed: the reference applied to a coordinate image, matched against every origin and d."""
    coord = torch.arange(h * w, dtype=torch.float32).view(1, h, w).expand(3, h, w).clone()
    blob, _ = _run(A, seed, size, coord, norm=False)
    out = blob['image'][0]
    for d in range(8):
        for y0 in range(h - size[0] + 1):
            for x0 in range(w - size[1] + 1):
                if torch.equal(aug_ref.apply_d(coord[0, y0:y0 + size[0], x0:x0 + size[1]], d), out):
                    return y0, x0, d
    raise AssertionError('no crop / element reproduces seed %d' % seed)


def main():
    A = _load_reference()
    rng = np.random.default_rng(20261015)
    H, W, S = 48, 40, (32, 32)
    img_hwc = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    soft = torch.from_numpy(rng.integers(0, 256, (6, H, W)).astype(np.float32) / 256)     # exact, compressible
    regs = torch.from_numpy(rng.integers(0, 40, (H, W)).astype(np.int64)).unsqueeze(0).long()
    image = torch.from_numpy(img_hwc).float().permute(2, 0, 1)         # basedata.py:70-72
    seeds, count = [], [0] * 8
    for s in range(1000):
        y0, x0, d = _decode(A, s, H, W, S)
        if count[d] < 2 or (len(seeds) < 24 and count[d] < 4):
            seeds.append((s, y0, x0, d))
            count[d] += 1
        if min(count) >= 2 and len(seeds) >= 24:
            break
    assert min(count) >= 2, count
    out = dict(small_img=img_hwc, small_soft=soft.numpy(), small_regs=regs[0].numpy().astype(np.int32),
               seeds=np.array([s[0] for s in seeds], np.int64),
               params=np.array([s[1:] for s in seeds], np.int32))
    imgs, masks, sups, nxt_py, nxt_t = [], [], [], [], []
    for s, *_ in seeds:
        blob, nxt = _run(A, s, S, image.clone(), soft.clone(), regs.clone())
        imgs.append(blob['image'].numpy())
        masks.append(blob['mask'].numpy())
        sups.append(blob['mask_sup'].numpy())
        nxt_py.append(nxt[0])
        nxt_t.append(nxt[1])
    out.update(small_image_out=np.stack(imgs), small_mask_out=np.stack(masks), small_sup_out=np.stack(sups),
               small_next_py=np.array(nxt_py, np.float64), small_next_torch=np.array(nxt_t, np.float32))
    # full size: a patterned 512 x 512 tile (compressible), crop 512 -> torchvision draws nothing
    yy, xx = np.meshgrid(np.arange(512), np.arange(512), indexing='ij')
    big = np.stack([(yy * 7 + xx * 13 + c * 29) % 256 for c in range(3)], -1).astype(np.uint8)
    blob, nxt = _run(A, 5, (512, 512), torch.from_numpy(big).float().permute(2, 0, 1))
    out.update(full_img=big, full_seed=np.int64(5), full_image_out=blob['image'].numpy(),
               full_next_py=np.float64(nxt[0]), full_next_torch=np.float32(nxt[1]))
    path = os.path.join(HERE, 'augment.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes), seeds %s, elements %s' % (path, os.path.getsize(path), [s[0] for s in seeds], count))


if __name__ == '__main__':
    main()
