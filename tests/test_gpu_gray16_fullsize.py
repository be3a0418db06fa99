"""bic_encode_gray16 at a size the automatic choice gives to the staged encoder (2048 rows x 16 planes =
32768 plane rows of 16384 columns): planes NULL, both streams, every plane's bit count and stream
against the oracle (on host threads)."""
import numpy as np
import pytest

from pybic import as_u64, stream_bytes

pytestmark = pytest.mark.gpu


def test_gray16_fullsize_auto(ctx, oracle):
    rows, cols = 2048, 16384
    i, j = np.mgrid[0:rows, 0:cols]
    noise = oracle.gen_bytes(0xF0116, rows * cols).reshape(rows, cols) % 7
    img = ((37 * i + 3 * j + noise) % 4096).astype(np.uint16)  # smooth12: planes 12-15 zero
    d = ctx.torch.from_numpy(img.astype(">u2").view(np.uint8).reshape(rows, 2 * cols)).to(ctx.dev)
    ctx.sync()
    ctx.prof_collect()
    ctx.prof_enable(True)
    try:
        ctx.prof_only("bitplanes_count")
        _, (og, bg), (oe, be) = ctx.encode_gray16(d, rows=rows, cols=cols, big_endian=True, store_planes=False)
        assert ctx.prof_collect()["bitplanes_count"][0] == 1  # the fused count pass, not the fallback
    finally:
        ctx.prof_only(None)
        ctx.prof_enable(False)
    exp = oracle.encode_planes_par(oracle.bitplanes_par(img, 16), cols, 1)
    for k in range(16):
        for coder, out, bits in ((0, og, bg), (1, oe, be)):
            eb, est = exp[(k, coder)]
            nb = int(as_u64(bits)[k])
            assert nb == eb, (k, coder)
            assert stream_bytes(out[k], nb) == est.tobytes(), (k, coder)
