/*
 * dkt_abi_data.h -- C ABI of libdkt_data.so (gfx950): the episode image transform of the image-dataset loader.
 *
 * One call turns B decoded RGB images (uint8, HWC, packed in one device pool) into the fp32 tensor [B, 3, S, S] the backbone reads, bit for bit
 * what Pillow + torchvision produce for the same parameters:
 *   1. bilinear resize of the source window (y0, x0, h, w) -- a crop is a new image: the filter support is clamped to the window -- to (rh, rw),
 *      Pillow's separable fixed-point resampler (horizontal pass first, uint8 intermediate, 22-bit coefficients);
 *   2. the S x S window of the result at (oy, ox);
 *   3. optionally ImageEnhance Brightness, Contrast, Color with per-image factors (jitter [B, 3], in that order);
 *   4. optionally a horizontal flip (flip [B], nonzero = flip);
 *   5. ToTensor (u8 / 255) and Normalize ((x - mean[c]) / std[c]), fp32 IEEE divisions.
 * Training episodes (RandomResizedCrop): window = the crop, (rh, rw) = (S, S), (oy, ox) = (0, 0).  Evaluation (Resize((a, a)) + CenterCrop(S)): window =
 * the whole image, (rh, rw) = (a, a), (oy, ox) = the centre offset.
 *
 * The per-image table is int64 [B, DKT_AUG_COLS], row-major:
 *   off (byte offset of the image in the pool), H, W, y0, x0, h, w, rh, rw, oy, ox, ws_off
 * Limits: 1 <= H, W <= DKT_AUG_MAX_SIDE; the window lies inside the image; 1 <= S <= DKT_AUG_MAX_S; S <= rh, rw <= DKT_AUG_MAX_SIDE; the output window lies
 * inside (rh, rw); off + H * W * 3 <= pool_bytes.  ws_off (coefficient tables, in 4-byte words) is written by dkt_augment_plan.
 *
 * Usage: dkt_augment_plan(table, B, S, &ws) validates the table on the host, fills its ws_off column and returns the workspace size; the caller copies the
 * table (as planned) to the device and calls dkt_augment_u8 with both copies: the host copy is validated again before any launch, the device copy is what
 * the kernels read (an entry that does not satisfy the limits there yields NaN for that image, never an access outside the pool).
 * Two launches (coefficient tables, then one workgroup per image), no host synchronisation.  Return values: DKT_OK / DKT_ERR_* of dkt_abi.h.
 */
#ifndef DKT_ABI_DATA_H
#define DKT_ABI_DATA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKT_DATA_ABI_VERSION 1

#define DKT_AUG_COLS 12
#define DKT_AUG_MAX_SIDE 16384
#define DKT_AUG_MAX_S 256

int dkt_data_abi_version(void);

/* validates table [B, DKT_AUG_COLS] (host memory), writes its ws_off column and *ws_bytes (the workspace dkt_augment_u8 needs) */
int dkt_augment_plan(int64_t* table, int B, int S, size_t* ws_bytes);

/* pool: device uint8 RGB images; table_host / table_dev: the planned table in host and device memory; jitter: device fp32 [B, 3] (Brightness, Contrast,
 * Color factors) or NULL; flip: device uint8 [B] or NULL; mean / std: host fp32 [3]; out: device fp32 [B, 3, S, S]; ws: device workspace of ws_bytes */
int dkt_augment_u8(const uint8_t* pool, size_t pool_bytes, const int64_t* table_host, const int64_t* table_dev, int B, const float* jitter,
                   const uint8_t* flip, int S, const float* mean, const float* std, float* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DKT_ABI_DATA_H */
