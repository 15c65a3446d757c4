"""GreyscaleWrapper.observation (gym_miniworld/wrappers.py:38-45) followed by the trainer's .float() (pytorch-a2c-ppo-acktr/envs.py:
119,128), restated in NumPy: the yardstick of every greyscale assertion of the suite.  NumPy only; no kernel of the library is
involved."""
import numpy as np


def grey_of_channels(r, g, b):
    """uint8 arrays -> float32: the wrapper's expression as NumPy evaluates it - float64 products, summed left to right - then the
    one rounding of .float()"""
    g64 = (0.30 * r + 0.59 * g) + 0.11 * b
    assert g64.dtype == np.float64
    return g64.astype(np.float32)


def grey_ref(rgb, layout):
    """uint8 frames [..., H, W, 3] ("HWC") -> float32 [..., H, W, 1]; [..., 3, W, H] ("CWH", after TransposeImage) -> [..., 1, W, H]"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8
    if layout == "HWC":
        return grey_of_channels(rgb[..., 0], rgb[..., 1], rgb[..., 2])[..., None]
    return grey_of_channels(rgb[..., 0, :, :], rgb[..., 1, :, :], rgb[..., 2, :, :])[..., None, :, :]
