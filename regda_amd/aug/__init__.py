"""GPU training augmentation of raw uint8 tiles.

augmentation: the reference's regda/aug/augmentation.py (target domain, `st.regda.*` TARGET_DATA_CONFIG);
albu: the albumentations pipeline of the source domain and evaluation (configs/To*.py).
`from_config(data_config)` builds the right one from the declarative transform lists of configs/.  Random scale and
rotation (`RandomScaleRotate`, albu's `ShiftScaleRotate`; `rgda_augment_affine`) are this project's
addition: a list entry `('RandomScaleRotate', dict(scale=(0.5, 2.0), degrees=15, prob=0.5))`."""
from . import albu, augmentation

_MAG = {'RandomCrop', 'RandomHorizontalFlip', 'RandomVerticalFlip', 'RandomRotate90', 'RandomScaleRotate', 'Normalize'}
_ALBU = {'RandomCrop', 'OneOf', 'HorizontalFlip', 'VerticalFlip', 'RandomRotate90', 'ShiftScaleRotate', 'Normalize',
         'ToTensor'}
_ALBU_ONLY = {'OneOf', 'HorizontalFlip', 'VerticalFlip', 'ShiftScaleRotate', 'ToTensor'}


def _is_albu(transforms):
    for t in transforms:
        if t[0] in _ALBU_ONLY or (t[0] == 'Normalize' and 'max_pixel_value' in t[1]):
            return True
    return False


def label_config(cfg):
    """The label table of a task config as from_config's keyword arguments: dict(offset, num_class, ignore_label) from
    the config's LABEL_OFFSET / NUM_CLASSES / IGNORE_LABEL, IsprsDA's (0, 6, -1) where a name is absent (the ISPRS
    modules do not set them).  st.regda.2rural / 2urban: (-1, 7, -1)."""
    return dict(offset=getattr(cfg, 'LABEL_OFFSET', 0), num_class=getattr(cfg, 'NUM_CLASSES', 6),
                ignore_label=getattr(cfg, 'IGNORE_LABEL', -1))


def from_config(data_config, rng=None, generator=None, offset=0, num_class=6, ignore_label=-1):
    """The pipeline of a loader config of configs/ (its `transforms` list): `st.regda.*` TARGET_DATA_CONFIG -> the
    reference (mag) pipeline with clamp; `To*` SOURCE_DATA_CONFIG -> the albumentations pipeline; EVAL / PSEUDO /
    TEST_DATA_CONFIG -> normalisation only.  rng / generator: see the two modules; offset / num_class / ignore_label:
    the label table (IsprsDA: 0, 6, -1; LoveDA: -1, 7, -1 -- `**label_config(cfg)` passes a config's).  Unknown
    transform names raise ValueError."""
    transforms = data_config['transforms']
    lab = dict(offset=offset, num_class=num_class, ignore_label=ignore_label)
    if _is_albu(transforms):
        def one(name):
            if name == 'HorizontalFlip':
                return albu.HorizontalFlip(True)
            if name == 'VerticalFlip':
                return albu.VerticalFlip(True)
            if name == 'RandomRotate90':
                return albu.RandomRotate90(True)
            raise ValueError('unknown albumentations transform %r' % (name,))
        out = []
        for t in transforms:
            name = t[0]
            if name not in _ALBU:
                raise ValueError('unknown albumentations transform %r' % (name,))
            if name == 'RandomCrop':
                out.append(albu.RandomCrop(*t[1]))
            elif name == 'OneOf':
                out.append(albu.OneOf([one(c) for c in t[1]], p=t[2]))
            elif name == 'Normalize':
                out.append(albu.Normalize(**t[1], always_apply=True))
            elif name == 'ToTensor':
                out.append(albu.ToTensor())
            elif name == 'ShiftScaleRotate':
                out.append(albu.ShiftScaleRotate(**t[1]))
            else:
                out.append(one(name))
        return albu.Compose(out, rng=rng, **lab)
    out = []
    for t in transforms:
        name = t[0]
        if name not in _MAG:
            raise ValueError('unknown transform %r' % (name,))
        if name == 'Normalize':
            out.append(augmentation.Normalize(**t[1]))
        elif name == 'RandomScaleRotate':
            out.append(augmentation.RandomScaleRotate(**t[1]))
        else:
            out.append(getattr(augmentation, name)(t[1]))
    return augmentation.Compose(out, rng=rng, generator=generator, **lab)
