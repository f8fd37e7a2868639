/* xpng_store_batch.h -- store a list of rasters of any sizes at once (libxpng.so; no counterpart in the reference).
 *
 * xpng_store_batch writes n files: file i is byte-identical to what xpng_store(mode, &pms[i], paths[i]) writes.  One level
 * (mode 1, 2 or 7) for the call.  Everything xpng_store decides on the host is decided here in the same order: level 7 and
 * single-pixel images and the flat RGB image of level 2 need no GPU; the other images are uploaded once as a staged batch
 * (xpnghip_images_*, include/xpng_hip.h), normalised and tested on the device, and the tile stage of all images of one (tile mode,
 * bytes per pixel) is ONE mixed-size device call: the serial entropy chains of all images run side by side, where a loop of
 * xpng_store calls runs them one image after the other.  A staged batch takes images in order until it holds 4096 of them or its
 * padded rasters (every row of every image at the widest image's pitch) would pass 2 GiB; an image that alone passes the budget
 * is a batch of its own.  One device; no MPx/s line is printed.
 *
 * Returns 0 on success.  Every image is validated before any work and NO file is written unless every image was validated and
 * encoded; n == 0, a NULL argument, an invalid image or a failed encode return 1 with no file written.  An I/O error while
 * writing returns 1 (files written before it stay).
 */
#ifndef XPNG_STORE_BATCH_H
#define XPNG_STORE_BATCH_H

#include "xpng.h"

#ifdef __cplusplus
extern "C" {
#endif

XPNG_CHECK _Bool xpng_store_batch(uint64_t mode, const xpng_t *pms, const char *const *paths, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif
