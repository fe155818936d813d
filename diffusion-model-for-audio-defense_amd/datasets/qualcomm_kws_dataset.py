"""The keyword-spotting dataset of the reference's second task (reference audio_models/RCNN_KWS/qualcomm_kws_dataset.py:7-96, the
version kws_adaptive_attack_eval.py:95 uses): `QualcommKeywordSpottingDataset(folder, usage, transform, classes)` over
<folder>/<class>/**/*.wav with the four keyword classes, and the `LoadAudio` / `FixAudioLength` transforms, written from their behaviour.

Differences from the reference:
  * WAV files are read by this package's loader (transforms.transforms_wav.read_wav: standard library + numpy, no librosa).  A file
    that is not sampled at 16 kHz is refused with a message, where librosa would resample it.
  * The reference takes its `Train` / `Valid` / `Test` slices (all but the last 125, the next 100, the last 25 files of every class)
    from the order of os.walk, which no two file systems agree on.  Here the paths of a class are sorted first, so the split is the
    same everywhere -- and therefore not the reference's on any particular machine."""
import os

from torch.utils.data import Dataset

from transforms.transforms_wav import FixAudioLength, LoadAudio

__all__ = ['CLASSES', 'QualcommKeywordSpottingDataset', 'LoadAudio', 'FixAudioLength']

CLASSES = 'hey_android, hey_snapdragon, hi_galaxy, hi_lumina'.split(', ')
USAGE_SLICES = {'Train': slice(None, -125), 'Valid': slice(-125, -25), 'Test': slice(-25, None)}


class QualcommKeywordSpottingDataset(Dataset):
    """items {'path', 'target'} (then whatever `transform` adds: LoadAudio gives 'samples' and 'sample_rate'); `usage` outside
    Train / Valid / Test takes every file, as in the reference."""

    def __init__(self, folder, usage='Train', transform=None, classes=CLASSES):
        super().__init__()
        for c in classes:
            if not os.path.isdir(os.path.join(folder, c)):
                raise FileNotFoundError('class folder %r is missing under %s (the dataset needs %s)' % (c, folder, ', '.join(classes)))
        data = []
        for target, c in enumerate(classes):
            paths = sorted(os.path.join(root, name) for root, _, files in os.walk(os.path.join(folder, c)) for name in files
                           if name.endswith('.wav'))
            data.extend((p, target) for p in paths[USAGE_SLICES.get(usage, slice(None))])
        self.classes = classes
        self.data = data
        self.transform = transform

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        path, target = self.data[index]
        data = {'path': path, 'target': target}
        if self.transform is not None:
            data = self.transform(data)
        return data
