"""BIC_OPT_RGB_PREDICT in numpy, on interleaved uint8 images [..., rows, cols, 3]: forward(img, ct, mode) =
U(img) = T_sp(T_ct(img)) -- colour_ref.forward per pixel, then sample_predict_ref.predict along the row on each of
the three channels separately (the left of column 0 is 0 in every row of every frame; G is differenced too) --
and inverse(z, ct, mode) undoes it: the per-channel prefix sum, then colour_ref.inverse. Plain integer arithmetic:
nothing here knows of planes, strips, lanes or Gray codes."""
import numpy as np

import colour_ref
from sample_predict_ref import predict, unpredict


def forward(img, ct, mode):
    v = colour_ref.forward(np.asarray(img, np.uint8), ct)
    # the row axis of a channel is the last but one of the interleaved image
    return np.moveaxis(predict(np.moveaxis(v, -1, -3), mode), -3, -1).copy()


def inverse(z, ct, mode):
    z = np.asarray(z, np.uint8)
    v = np.moveaxis(unpredict(np.moveaxis(z, -1, -3), mode), -3, -1).copy()
    return colour_ref.inverse(v, ct)
