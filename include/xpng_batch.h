/* xpng_batch.h -- load a list of .xpng files of any sizes at once (libxpng.so; no counterpart in the reference).
 *
 * xpng_load_batch reads n files and fills out[0 .. n): out[i] holds exactly what xpng_load(paths[i], &out[i]) returns
 * (out[i].p malloc()ed, the caller frees each).  Level-7 files and whole-image single-colour files are answered on the host.
 * The other files are grouped by (tile mode, bytes per pixel) and every group is decoded by ONE mixed-size device call
 * (xpnghip_decode_mixed, include/xpng_hip.h): the serial entropy chains of all its images run side by side, where a loop of
 * xpng_load calls runs them one image after the other.  One device.
 *
 * Returns 0 on success.  If any file cannot be read or decoded the call returns 1, frees what it allocated and leaves every
 * out[i].p NULL.
 */
#ifndef XPNG_BATCH_H
#define XPNG_BATCH_H

#include "xpng.h"

#ifdef __cplusplus
extern "C" {
#endif

_Bool xpng_load_batch(const char *const *paths, uint64_t n, xpng_t *out);

#ifdef __cplusplus
}
#endif
#endif
