"""The reference the training-augmentation tests measure against (not a test module): the four steps of dat_loader.augment_host
restated independently — Pillow itself for step 1 (`img.crop(box).resize((Wo, Ho))`), plain per-pixel loops over numpy float32 scalars
for steps 2-4 (every product and sum is one fp32 operation, so nothing can be fused):
    blend(x, m, f) = trunc_to_u8(clamp(f * x + (1 - f) * m, 0, 255))        gray(p) = trunc_to_u8((0.2989 r + 0.587 g) + 0.114 b)
    2. brightness blend(x, 0, b);  3. contrast blend(x, mean, c), mean = float32(exact integer sum of gray after step 2 / (Ho * Wo),
    the division in double precision);  4. saturation blend(x, gray(pixel after step 3), s)."""
import numpy as np

F = np.float32


def blend(x, m, f):
    v = F(F(f) * F(x)) + F(F(F(1) - F(f)) * F(m))
    v = F(0) if v < F(0) else (F(255) if v > F(255) else v)
    return int(v)                       # truncation; 0 <= v <= 255


def gray(r, g, b):
    return int(F(F(F(0.2989) * F(r)) + F(F(0.587) * F(g))) + F(F(0.114) * F(b)))


def step1(img, crop, out_hw):
    import PIL.Image
    x0, y0, x1, y1 = (int(v) for v in crop)
    return np.asarray(PIL.Image.fromarray(img).crop((x0, y0, x1, y1)).resize((int(out_hw[1]), int(out_hw[0]))))


def jitter(img, factors):
    """steps 2-4 on a uint8 [H, W, 3] image"""
    fb, fc, fs = (F(v) for v in factors)
    H, W, _ = img.shape
    p = [[[blend(int(v), 0, fb) for v in img[y, x]] for x in range(W)] for y in range(H)]
    total = sum(gray(*p[y][x]) for y in range(H) for x in range(W))               # a Python integer: exact
    mean = F(np.float64(total) / np.float64(H * W))
    out = np.empty((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            q = [blend(v, mean, fc) for v in p[y][x]]
            gq = gray(*q)
            out[y, x] = [blend(v, gq, fs) for v in q]
    return out


def augment(img, crop, factors, out_hw):
    return jitter(step1(img, crop, out_hw), factors)
