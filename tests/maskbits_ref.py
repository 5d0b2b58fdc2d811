"""The one-bit ReLU pattern of a block output, restated in NumPy (lp_bn_add_act_bits, include/lp_hip.h): one byte per (pixel, 8-channel group), bit j of
byte g = channel 8 g + j, set where the 16-bit HI plane word of that element is > 0 -- sign clear and magnitude non-zero."""
import numpy as np


def positive(words):
    """the predicate on uint16 plane words (bf16 or fp16 alike): (w - 1) < 0x7fff in unsigned arithmetic"""
    w = np.asarray(words).astype(np.uint16).astype(np.uint32)
    return ((w - np.uint32(1)) & np.uint32(0xffffffff)) < np.uint32(0x7fff)


def pack(words):
    """uint16 words [..., C] (C % 8 == 0) -> uint8 [..., C / 8]"""
    w = np.asarray(words)
    assert w.shape[-1] % 8 == 0
    return np.packbits(positive(w), axis=-1, bitorder='little')


def plane_words(hi):
    """the int16 plane tensor a wrapper returned -> its uint16 words on the host"""
    return hi.detach().cpu().contiguous().numpy().view(np.uint16)
