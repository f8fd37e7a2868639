/* xpng_store_tensors.h -- store a list of DEVICE buffers of any sizes as .xpng files (libxpng.so; no counterpart in the reference).
 *
 * xpng_store_tensors is xpng_store_batch (xpng_store_batch.h) for images that live on the GPU in the form a model writes: planar or
 * interleaved, RGB or BGR, 3 or 4 channels per image, uint8, f16, bf16 or f32.  Image i is d_bufs[i], a tight device buffer of
 * channels[i] * w_i * h_i elements (dims = n pairs {w, h}) aligned to its element; layout, dtype, scale and bias are those of
 * xpnghip_images_begin_device (include/xpng_hip.h), where the quantisation rule is written down:
 *     v = clamp-and-round-half-to-even(fmaf(x, scale[c], bias[c]))      dtype 0: the buffer holds the bytes, no constants
 * File i is byte for byte what xpng_store(mode, ...) writes for the quantised interleaved R,G,B[,A] raster of image i.  The
 * buffers never cross to the host: a staged batch is filled from them by one kernel queued on `stream` (a stream of `device`, or
 * NULL; the call is ordered behind the work queued there), and everything xpng_store decides - normalize_RGBA, the single colour
 * of level 2, RGBA at level 2 -> level 1, RGBA narrower or shorter than 4 px -> level 7, the raw fallback - is decided as
 * xpng_store_batch decides it, from what the device reports.  A raster comes back to the host only for a file that holds it raw
 * (level 7, one pixel, the fallbacks).  The list is cut into staged batches as xpng_store_batch cuts it.
 *
 * Returns 0 on success.  NO file is written unless every image was staged and encoded; n == 0, a NULL argument, a bad size,
 * channel count, layout, dtype or constant, a misaligned buffer or a failed encode return 1 with no file written
 * (xpnghip_last_error() has the reason of a refused staging).  An I/O error while writing returns 1 (files written before it stay).
 */
#ifndef XPNG_STORE_TENSORS_H
#define XPNG_STORE_TENSORS_H

#include "xpng.h"

#ifdef __cplusplus
extern "C" {
#endif

XPNG_CHECK _Bool xpng_store_tensors(uint64_t mode, uint64_t n, const void *const *d_bufs, const uint64_t *dims, const uint8_t *channels,
                                    uint32_t layout, uint32_t dtype, const float *scale, const float *bias, int device, void *stream,
                                    const char *const *paths);

#ifdef __cplusplus
}
#endif
#endif
