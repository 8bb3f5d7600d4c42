"""The overlay of include/srad.h (srad_overlay_rgb) as an index loop in numpy, pixel by pixel: the oracle of
tests/test_gpu_overlay.py and tests/test_gpu_predict_source_frame.py.  No GPU, no library."""
import numpy as np


def overlay_ref(src, maps, masks, lut, scale, radius, colour):
    """src u8 [n,H,W,Cs] (Cs 1 or 3), maps f32 [n,H,W], masks u8 [n,H,W], lut u8 [256,4], scale a float32 -> u8 [n,H,W,3]."""
    n, H, W, Cs = src.shape
    scale = np.float32(scale)
    out = np.empty((n, H, W, 3), dtype=np.uint8)
    for i in range(n):
        for y in range(H):
            for x in range(W):
                contour = False
                if radius > 0 and masks[i, y, x]:
                    for yy in range(y - radius, y + radius + 1):
                        for xx in range(x - radius, x + radius + 1):
                            if yy < 0 or yy >= H or xx < 0 or xx >= W or masks[i, yy, xx] == 0:
                                contour = True
                if contour:
                    out[i, y, x] = colour
                    continue
                with np.errstate(over="ignore", invalid="ignore"):
                    q = np.float32(maps[i, y, x]) * scale      # one fp32 multiply
                level = 255 if q >= 255 else (int(q) if q > 0 else 0)      # NaN fails both comparisons
                r, g, b, a = (int(v) for v in lut[level])
                for c, t in enumerate((r, g, b)):
                    v = int(src[i, y, x, c if Cs == 3 else 0])
                    out[i, y, x, c] = (v * (255 - a) + t * a + 127) // 255
    return out
