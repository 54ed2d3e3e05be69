"""Data-side config of the LoveDA Rural -> Urban task: the attribute surface of the reference's configs/ToURBAN.py
(names and values).  Paths point at the LoveDA folders of the public release (1024 x 1024 PNG tiles; decoding them is
not part of this build), so the augmentation pipelines are described declaratively instead of through albumentations
objects, as in configs/ToPotsdam.py.  LoveDA masks store class + 1 (0 = no-data): the label table of these tasks is
offset -1, 7 classes, ignore -1 (the reference's regda/datasets/loveda.py)."""
DATASETS = 'LoveDA'
TARGET_SET = 'Urban'
MEAN = (73.53223948, 80.01710095, 74.59297778)
STD = (41.5113661, 35.66528876, 33.75830885)

source_dir = dict(image_dir=['data/LoveDA/Train/Rural/images_png'], mask_dir=['data/LoveDA/Train/Rural/masks_png'])
target_dir = dict(image_dir=['data/LoveDA/Val/Urban/images_png'], mask_dir=[None])
val_dir = dict(image_dir=['data/LoveDA/Train/Urban/images_png'], mask_dir=['data/LoveDA/Train/Urban/masks_png'])
test_dir = dict(image_dir=['data/LoveDA/Test/Urban/images_png'], mask_dir=[None])

_TRAIN_AUG = [('RandomCrop', (512, 512)), ('OneOf', ('HorizontalFlip', 'VerticalFlip', 'RandomRotate90'), 0.75),
              ('Normalize', dict(mean=MEAN, std=STD, max_pixel_value=1)), ('ToTensor',)]
_EVAL_AUG = [('Normalize', dict(mean=MEAN, std=STD, max_pixel_value=1)), ('ToTensor',)]

SOURCE_DATA_CONFIG = dict(image_dir=source_dir['image_dir'], mask_dir=source_dir['mask_dir'], transforms=_TRAIN_AUG,
                          CV=dict(k=10, i=-1), training=True, batch_size=8, num_workers=4)
TARGET_DATA_CONFIG = dict(image_dir=target_dir['image_dir'], mask_dir=target_dir['mask_dir'], transforms=_TRAIN_AUG,
                          CV=dict(k=10, i=-1), training=True, batch_size=8, num_workers=4)
PSEUDO_DATA_CONFIG = dict(image_dir=target_dir['image_dir'], mask_dir=target_dir['mask_dir'], transforms=_EVAL_AUG,
                          CV=dict(k=10, i=-1), training=False, batch_size=1, num_workers=1)
EVAL_DATA_CONFIG = dict(image_dir=val_dir['image_dir'], mask_dir=val_dir['mask_dir'], transforms=_EVAL_AUG,
                        CV=dict(k=10, i=-1), training=False, batch_size=1, num_workers=1)
TEST_DATA_CONFIG = dict(image_dir=test_dir['image_dir'], mask_dir=test_dir['mask_dir'], transforms=_EVAL_AUG,
                        CV=dict(k=10, i=-1), training=False, batch_size=1, num_workers=1)
