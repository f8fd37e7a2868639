/* xpng_region.h -- region decode of an .xpng file, exported by libxpng.so next to the reference's API (include/xpng.h).
 *
 * Not part of the reference's surface, so it lives in its own header: xpng.h declares exactly what the reference declares.
 */
#ifndef XPNG_REGION_H
#define XPNG_REGION_H

#include "xpng.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Decode the w x h rectangle at (x, y) of the image in file `xpng` into pm: pm->w = w, pm->h = h, pm->A from the file,
 * pm->s = w * h * (3 + A), pm->p malloc()ed (the caller frees it), rows back to back.  0 = success, 1 = failure (as xpng_load;
 * re-entrant like it).  A rectangle that is empty or leaves the image fails.  Level-7 files and whole-image single-colour files
 * are cropped on the host and need no GPU; levels 1 and 2 decode only the tiles the rectangle touches, on one GPU
 * (xpnghip_decode_region, include/xpng_hip.h). */
XPNG_CHECK _Bool xpng_load_region(const char *xpng, uint64_t x, uint64_t y, uint64_t w, uint64_t h, xpng_t *pm);

#ifdef __cplusplus
}
#endif
#endif
