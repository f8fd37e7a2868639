/* xpng_hip.h -- C-ABI of libxpng_hip.so: the MI355X tile codec behind xpng_store / xpng_load.
 *
 * This is the "inner boundary" of SURVEY.md §8(b): it replaces the two pthread fan-outs of the
 * reference driver,
 *     spawn_and_wait(T, &d, 0, enc_1_th | enc_2_th)   reference libxpng.c:758
 *     spawn_and_wait(T, &d, 0, dec_1_th | dec_2_th)   reference libxpng.c:983
 * i.e. "given the raster and the tile table, produce every tile's blob" and the reverse.  Plain
 * pointers and sizes only; no C++ or torch types.  All functions return 0 on success, non-zero on
 * failure (the reference's _Bool convention, libxpng.c:729-731); xpnghip_last_error() describes the
 * last failure of the calling thread.  There is NO CPU fallback: without a usable HIP device every
 * compute entry point fails.
 *
 * Threading: like the reference (no globals; every call spawns and joins its own workers, until_fork/4_letters.c:9-17) the
 * host-buffer and staged-image entry points are RE-ENTRANT: any number of host threads may call them at the same time; each
 * call works on a context, a stream and staging buffers of its own (taken from a pool of idle ones and given back), and no
 * lock is held while a call runs.  A device-resident context (xpnghip_ctx) is a single-queue object owned by its caller.
 *
 * Environment read by the release library (each selects between forms that produce the same bytes):
 * XPNG_DEVICE, XPNG_GPUS, XPNG_WIDE_RANS, XPNG_NARROW_RANS.  Switches that
 * exist for timing studies (kernel knock-outs, LDS pads, stamps, the wave probe, fake devices) are compiled only into
 * libxpng_hip_probes.so (`make probes`).
 */
#ifndef XPNG_HIP_H
#define XPNG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XPNGHIP_ABI_VERSION 2   /* 2: the staged image is a handle (re-entrant xpng_store); T == 0 means one device */

int xpnghip_abi_version(void);
int xpnghip_device_count(void);          /* visible HIP devices; 0 when none / no runtime */
const char *xpnghip_last_error(void);

/* ---- host-buffer entry points: what the host C driver (xpng_store_T / xpng_load_T) calls ----------
 *
 * xpnghip_encode_tiles  <->  libxpng.c:758 + the concatenation loop libxpng.c:764-769.
 *   raster: normalised interleaved raster, w*h*pxsz bytes (pxsz 3 or 4), host memory.
 *   mode:   1 (enc_1_th, RGB and RGBA) or 2 (enc_2_th, RGB only).
 *   *blobs: malloc()ed concatenation of all tile blobs in tile order (caller frees with free()).
 * xpnghip_decode_tiles  <->  libxpng.c:982-983.
 *   blobs:  the file body after the 8-byte header; tile sizes are walked serially as the reference does.
 *   raster: caller-allocated w*h*pxsz bytes, filled completely.
 */
int xpnghip_encode_tiles(int mode, const uint8_t *raster, uint64_t w, uint64_t h, int pxsz,
                         uint8_t **blobs, uint64_t *blobs_len);
int xpnghip_decode_tiles(int mode, const uint8_t *blobs, uint64_t blobs_len, uint64_t w, uint64_t h,
                         int pxsz, uint8_t *raster);
/* The same with the reference's worker count T (libxpng.c:146-151: T workers share the tile cursor, T = min(T, N)).  Here a
 * worker is a DEVICE of this process: T >= 1 uses min(T, visible devices, N) of them.  T == 0 (the reference's "auto") uses
 * ONE device: the multi-device path has not yet passed a byte-parity run on real peer devices, so it is opt-in (T > 1, or
 * XPNG_GPUS=<n> for T == 0).  Every device codes one contiguous, pixel-weighted tile range from its own band of the raster;
 * for the encode the blob ranges are gathered on the first device by peer copies (xGMI; peer access is queried and enabled
 * once per device pair) for the concatenation of libxpng.c:764-769, then copied to the host once.  When a pair of devices has
 * no peer access the copies are staged through host memory by the runtime: the call still succeeds and xpnghip_last_error()
 * then holds a note that starts with "note:".  The bytes do not depend on T (tiles are coded independently).
 * xpnghip_encode_tiles / xpnghip_decode_tiles are T = 1.  XPNG_DEVICE=<n> selects the first device (default 0); the
 * caller's current HIP device is restored before returning. */
int xpnghip_encode_tiles_T(uint64_t T, int mode, const uint8_t *raster, uint64_t w, uint64_t h, int pxsz,
                           uint8_t **blobs, uint64_t *blobs_len);
int xpnghip_decode_tiles_T(uint64_t T, int mode, const uint8_t *blobs, uint64_t blobs_len, uint64_t w, uint64_t h,
                           int pxsz, uint8_t *raster);
/* number of devices such a call would use for a w x h image (0 = no usable device) */
int xpnghip_devices_for(uint64_t T, uint64_t w, uint64_t h);
/* host-only (needs no device): the contiguous tile ranges a call on D devices would use; ranges[2k], ranges[2k+1] = [r0, r1) of
 * device k.  Returns the number of ranges (= min(D, tiles)), -1 on bad arguments or cap too small. */
int xpnghip_shard_ranges(uint64_t w, uint64_t h, int D, uint64_t *ranges, int cap);
/* Optional: gives every pooled idle object (contexts with their workspaces, staging buffers) back to the runtime.  Must not
 * run concurrently with other calls into this library. */
void xpnghip_shutdown(void);

/* ---- staged image: upload once, normalise and test on the device ------------------------------------
 *
 * xpng_store's pre-passes over the whole raster, moved off the host:
 *   xpnghip_image_begin          <->  normalize_RGBA, libxpng.c:688-721 (called at libxpng.c:733).  Uploads the caller's
 *                                     raster (w*h*pxsz_in bytes, host memory) and, for RGBA, applies the rule on the device:
 *                                     hidden colours under alpha 0 -> those pixels zeroed; no translucent pixel -> repacked
 *                                     to RGB.  *pxsz_out = 3 or 4 = bytes per pixel of the staged (normalised) raster.
 *   xpnghip_image_single_colour  <->  the whole-image test of libxpng.c:741-753: *single = 1 if every pixel equals the first.
 *   xpnghip_image_encode         <->  libxpng.c:758-769 on the staged raster (as xpnghip_encode_tiles).
 *   xpnghip_image_fetch               staged raster -> host (w*h*pxsz_out bytes): the level-7 and single-colour outputs.
 *   xpnghip_image_end                 hands the staging object back (always call it once begin has returned 0).
 * Every xpng_store call in flight stages its own image: begin returns a handle, the other calls take it.  Handles of different
 * threads are independent (the reference is re-entrant); one handle is used by one thread at a time.
 * xpnghip_normalize_device is the same rule for a caller whose RGBA raster already lives in HBM (on the caller's current
 * device): *rewritten = 0 means the raster is already normal (use d_rgba), 1 means d_out (npx * *pxsz_out bytes,
 * caller-allocated npx*4) holds it.  It synchronises `stream` once (the two flags come back to the host). */
typedef struct xpnghip_image xpnghip_image;
int xpnghip_image_begin(xpnghip_image **img, const uint8_t *raster, uint64_t w, uint64_t h, int pxsz_in, int *pxsz_out);
int xpnghip_image_single_colour(xpnghip_image *img, int *single);
int xpnghip_image_encode(xpnghip_image *img, int mode, uint8_t **blobs, uint64_t *blobs_len);
int xpnghip_image_encode_T(xpnghip_image *img, uint64_t T, int mode, uint8_t **blobs, uint64_t *blobs_len);  /* T devices, as xpnghip_encode_tiles_T */
int xpnghip_image_fetch(xpnghip_image *img, uint8_t *dst);
void xpnghip_image_end(xpnghip_image *img);
int xpnghip_normalize_device(const void *d_rgba, uint64_t npx, void *d_out, int *pxsz_out, int *rewritten, void *stream);

/* ---- staged batch: the staged image for a list of images of any sizes (what xpng_store_batch calls) ----------
 *   xpnghip_images_begin          uploads rasters[i] (dims = nimg pairs {w, h}; pxsz_in[i] = 3 or 4; host memory, tight) once, each
 *                                 16-byte aligned on the device, and applies normalize_RGBA to every RGBA input: one launch takes
 *                                 the two flags of every image, a second applies the rewrite each image's flags ask for, and the
 *                                 flags are read back once for the call.  pxsz_out[i] = bytes per pixel of the normalised raster.
 *                                 The caller's rasters are free again when it returns.  nimg = 1 .. 4096.
 *   xpnghip_images_single_colour  the whole-image test of libxpng.c:741-753 for all images in one launch: nimg flags.
 *   xpnghip_images_encode         modes[i] = 0 (skip), 1 or 2 (RGB only).  The images with a non-zero mode are grouped by (mode,
 *                                 normalised pxsz) - at most three groups - and each group is ONE tight-form call of
 *                                 xpnghip_encode_varsize_device_batch on a mixed context created for the call.  blobs[i] is
 *                                 malloc()ed (caller frees) and lens[i] its length; skipped images get NULL / 0.  On failure
 *                                 everything allocated is freed and every blobs[i] is NULL.  An RGBA image narrower or shorter
 *                                 than 4 px must be skipped (store it at level 7).
 *   xpnghip_images_first_pixel    after xpnghip_images_single_colour: the first pixel of normalised raster i (pxsz_out[i] bytes).
 *                                 It came back with the flags, so the single-colour file of level 2 costs no fetch of a raster.
 *   xpnghip_images_fetch          normalised raster i -> host, tight (w_i * h_i * pxsz_out[i] bytes).
 *   xpnghip_images_end            frees the handle (always call it once begin has returned 0; NULL is allowed).
 * One device (XPNG_DEVICE; T and XPNG_GPUS do not apply).  DEVICE MEMORY of a handle: the rasters, 3 B per pixel of the RGBA inputs
 * for the repack, and during encode per group the blob bounds (the raw size) and the mixed context's workspace (xpng_hip.h below):
 * size the list accordingly (xpng_store_batch keeps a call under 4096 images and 2 GiB of padded rasters).  Handles are independent:
 * any number of threads may each use their own at the same time; one handle is used by one thread at a time. */
typedef struct xpnghip_images xpnghip_images;
int xpnghip_images_begin(xpnghip_images **h, uint32_t nimg, const uint8_t *const *rasters, const uint64_t *dims,
                         const uint8_t *pxsz_in, uint8_t *pxsz_out);
int xpnghip_images_single_colour(xpnghip_images *h, uint8_t *single);
int xpnghip_images_encode(xpnghip_images *h, const uint8_t *modes, uint8_t **blobs, uint64_t *lens);
int xpnghip_images_first_pixel(xpnghip_images *h, uint32_t i, uint8_t *px);
int xpnghip_images_fetch(xpnghip_images *h, uint32_t i, uint8_t *dst);
void xpnghip_images_end(xpnghip_images *h);
/* host-only (needs no device): where xpng_store_batch cuts a list of n images (dims = n pairs {w, h}, pxsz[i] = bytes per pixel as
 * handed in) into staged batches.  A batch takes images in order until it holds max_images of them or its padded rasters - every
 * row of every image at the widest image's pitch - would pass max_bytes; an image that alone passes the budget is a batch of its
 * own.  starts[k] = first image of batch k; returns the number of batches, -1 on bad arguments or when cap is too small. */
int xpnghip_batch_cuts(uint32_t n, const uint64_t *dims, const uint8_t *pxsz, uint32_t max_images, uint64_t max_bytes,
                       uint32_t *starts, int cap);

/* ---- device-resident entry points (bench, multi-GPU sharding, pipelines) ---------------------------
 *
 * A context owns the tile table (libxpng.c:51-83) and every intermediate buffer for one raster
 * geometry on one device, so the hot path itself performs no allocation and no host sync except the
 * final 8-byte length read-back.  `stream` is a hipStream_t passed as void* (NULL = the context's own).
 * A context is a single-queue object: the calls made on one context must be ordered (issue them on one stream).
 * Its buffers are reused from call to call, and the decode workspace lives inside the encode stream scratch.
 * Use one context per pipeline slot to overlap work.
 */
typedef struct xpnghip_ctx xpnghip_ctx;

int xpnghip_ctx_create(xpnghip_ctx **ctx, int device, uint64_t w, uint64_t h, int pxsz);
/* Same, sized for up to `batch` rasters of this geometry per launch.  The entropy stage is one serial chain per
 * (tile, stream), so a single 4096^2 image (81 tiles) cannot fill 256 CUs; a batched launch runs the chains of all
 * images side by side (virtual tile = image * N + tile) at the latency of one image. */
int xpnghip_ctx_create_batch(xpnghip_ctx **ctx, int device, uint64_t w, uint64_t h, int pxsz, uint32_t batch);
/* Same, with workspace for tiles [r0, r1) only: a rank that codes one tile range of a large raster (multi-GPU sharding)
 * pays HBM for its share, not for the whole image.  Encode / decode calls must stay inside [r0, r1). */
int xpnghip_ctx_create_range(xpnghip_ctx **ctx, int device, uint64_t w, uint64_t h, int pxsz, uint32_t batch,
                             uint64_t r0, uint64_t r1);
uint32_t xpnghip_ctx_batch(const xpnghip_ctx *ctx);
void xpnghip_ctx_destroy(xpnghip_ctx *ctx);
uint64_t xpnghip_ctx_tile_count(const xpnghip_ctx *ctx);
/* tile i -> {x, y, w, h} (pixels); returns non-zero if i is out of range */
int xpnghip_ctx_tile(const xpnghip_ctx *ctx, uint64_t i, uint64_t xywh[4]);
/* upper bound of the concatenated blobs of tiles [t0, t1) (raw fallback bound: sum(w*h*pxsz + 4)).  On a mixed context t0 and t1
 * index the concatenated table: image i's blob buffer needs blob_bound(first_tile(i), first_tile(i + 1)). */
uint64_t xpnghip_ctx_blob_bound(const xpnghip_ctx *ctx, uint64_t t0, uint64_t t1);
/* the sum of all device memory the context holds now: what it was created with and everything its calls have allocated since -
 * planes and scratch, the level-2 and wide-form tables, the decode tables, staging rasters, the host wrappers' buffers */
uint64_t xpnghip_ctx_workspace_bytes(const xpnghip_ctx *ctx);

/* Encode tiles [t0, t1) of the device raster `d_raster` (full w*h*pxsz image, device pointer) into
 * `d_blobs` (device pointer, capacity >= xpnghip_ctx_blob_bound).  On return *blobs_len is the byte
 * count (one stream sync).  Pass blobs_len == NULL to skip the sync and read the length later with
 * xpnghip_ctx_last_blobs_len() after synchronising the stream yourself. */
int xpnghip_encode_device(xpnghip_ctx *ctx, int mode, const void *d_raster, uint64_t t0, uint64_t t1,
                          void *d_blobs, uint64_t *blobs_len, void *stream);
uint64_t xpnghip_ctx_last_blobs_len(xpnghip_ctx *ctx);
/* Batched form: nimg <= batch device rasters in, nimg device blob buffers out (host arrays of device pointers);
 * blobs_len, if not NULL, receives nimg lengths after one stream sync. */
int xpnghip_encode_device_batch(xpnghip_ctx *ctx, int mode, const void *const *d_rasters, uint32_t nimg, uint64_t t0,
                                uint64_t t1, void *const *d_blobs, uint64_t *blobs_len, void *stream);
uint64_t xpnghip_ctx_last_blobs_len_at(xpnghip_ctx *ctx, uint32_t img);

/* Decode tiles [t0, t1).  d_blobs holds their concatenated blobs (device); tile_off[i - t0] is the byte
 * offset of tile i's blob inside d_blobs (host array from the serial size walk, libxpng.c:982), or tile_off == NULL:
 * the walk is done on the device (one lane per image follows the 24-bit sizes), so a caller whose blobs live in HBM never
 * copies them back to find the offsets.
 * Blob buffers handed to these entry points need 64 readable bytes behind their contents (their last words are fetched in
 * aligned blocks); the host-side wrappers (xpnghip_encode_tiles / xpnghip_decode_tiles / libxpng.so) allocate that
 * themselves.  A WHOLE raster needs no slack: every kernel that reads one in 16-byte pieces clamps at w*h*pxsz bytes.  A caller
 * that hands over only a BAND of the raster behind a virtual base pointer (a rank coding tile range [t0, t1) keeps rows
 * [y0, y1) and passes band - y0*w*pxsz) must keep 16 readable bytes behind the band's last row unless the band ends with the
 * raster: the clamp is at the end of the whole raster, so the last 16-byte piece of the band's last row may reach up to 15 bytes
 * into the next row (bench.py and the multi-device wrappers allocate a spare 16 bytes for this). */
int xpnghip_decode_device(xpnghip_ctx *ctx, int mode, const void *d_blobs, uint64_t blobs_len,
                          const uint64_t *tile_off, uint64_t t0, uint64_t t1, void *d_raster, void *stream);

/* Batched form: blobs_len[nimg] = bytes of each blob buffer; tile_off holds nimg * (t1 - t0) offsets, image-major, each
 * relative to its image's blob buffer. */
int xpnghip_decode_device_batch(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                const uint64_t *tile_off, uint64_t t0, uint64_t t1, void *const *d_rasters, void *stream);
/* The reference decoder trusts the file; this one validates every tile header (lengths, offsets, symbol counts) on the
 * device before using it.  Synchronises `stream` and returns 0 if the last decode accepted every tile, 1 if some tile
 * was rejected (its pixels are left untouched), -1 on a HIP error.  xpnghip_decode_tiles checks it for you. */
int xpnghip_ctx_decode_status(xpnghip_ctx *ctx, void *stream);

/* ---- region decode: only the tiles a crop rectangle touches (INTEGRATION.md "Region decode") ----------
 * A rectangle rect = {x, y, w, h} (pixels) is valid when w > 0, h > 0, x + w <= image width and y + h <= image height.  An
 * invalid rectangle is rejected before any device work: the call fails, xpnghip_last_error() says why, nothing is written.
 * Each tile is coded independently, so a crop is decoded from the tiles it intersects and nothing else.  The selected tiles are
 * reconstructed into a per-context staging raster (allocated on first use, grown on demand: nimg x the largest tile-aligned
 * bounding box of the selected tiles of a call), and the rectangle is copied from there into the caller's buffer.
 *
 * host-only (needs no device): the tiles of a w x h image that rect intersects, ascending; returns their count, -1 on an empty /
 * out-of-image rect or when cap is too small */
int xpnghip_region_tiles(uint64_t w, uint64_t h, const uint64_t rect[4], uint32_t *tiles, int cap);
/* Host buffers, one device (T and XPNG_GPUS do not apply).  blobs = the file body after the 8-byte header; the tile sizes are
 * walked on the host and only the bytes from the first selected tile's blob to the end of the last one are uploaded.
 * out = rect[2] * rect[3] * pxsz bytes, rows back to back. */
int xpnghip_decode_region(int mode, const uint8_t *blobs, uint64_t blobs_len, uint64_t w, uint64_t h, int pxsz,
                          const uint64_t rect[4], uint8_t *out);
/* Device-resident batch on a context created over the whole tile table: rects = nimg * 4 (one rectangle PER IMAGE);
 * d_outs[i] receives image i's crop, rect[2] * pxsz bytes per row at row pitch out_bpr (>= rect[2] * pxsz): bytes of a row
 * beyond rect[2] * pxsz and everything behind the last row are not written.  tile_off == NULL: the size walk runs on the device;
 * otherwise it holds nimg * N offsets (the FULL tile table of every image, image-major, relative to each image's blob buffer;
 * entries of tiles outside the rectangle are not read).  Tile headers are validated as in xpnghip_decode_device_batch, and
 * xpnghip_ctx_decode_status reports on this launch (a rejected tile leaves its part of the crop undefined). */
int xpnghip_decode_region_device_batch(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                       uint32_t nimg, const uint64_t *tile_off, const uint64_t *rects,
                                       void *const *d_outs, uint64_t out_bpr, void *stream);

/* ---- mixed-size batches: images of different sizes in one device call (INTEGRATION.md "Mixed-size batches") ----------
 * A mixed context decodes (xpnghip_decode_mixed_device_batch) and encodes (xpnghip_encode_varsize_device_batch) its batch as a
 * whole.  The constructor allocates what a decode needs; the encode workspace is allocated by the first encode call.  It holds nimg images of one pixel size (pxsz 3 or 4) whose widths and heights differ:
 * dims = nimg pairs {w, h}.  Its tile table is the concatenation of the images' tile tables, M = sum of their tile counts entries
 * (M must fit in 32 bits; w, h <= 1 << 24; nimg <= 4096), and every workspace is sized from M and the summed pixel counts.
 * xpnghip_ctx_tile_count returns M and xpnghip_ctx_tile walks the concatenated table; xpnghip_ctx_mixed_first_tile(ctx, i) is the
 * table index of image i's first tile, for i == nimg it is M (so image i has first_tile(i + 1) - first_tile(i) tiles); beyond
 * nimg, or on an ordinary context, it returns UINT64_MAX.  xpnghip_ctx_batch returns nimg.  The entry points of an ordinary context
 * (xpnghip_encode_device[_batch], xpnghip_m1_transform_device[_batch], the tile-range decode and the region decode) refuse a mixed
 * context with an error text before any device work. */
int xpnghip_ctx_create_mixed(xpnghip_ctx **ctx, int device, const uint64_t *dims, uint32_t nimg, int pxsz);
uint64_t xpnghip_ctx_mixed_first_tile(const xpnghip_ctx *ctx, uint32_t image);
/* One launch over all M tiles (an explicit work list sorted by decreasing pixel count; unsplit).  One tile mode per
 * call (mode 2: RGB only).  d_blobs[i] / blobs_len[i]: image i's tile body on the device (64 readable bytes behind it, as above).
 * tile_off == NULL: the size walk runs on the device, one lane per image; otherwise tile_off holds M offsets, image after image,
 * each relative to its own blob buffer.
 *   out_bpr != 0  padded batch: every d_outs[i] (16-byte aligned) is written at this one row pitch, >= (widest image) * pxsz.  The
 *                 kernels reconstruct straight into the caller's buffers; bytes of a row past w_i * pxsz and rows from h_i on
 *                 are not written.
 *   out_bpr == 0  tight rasters: d_outs[i] receives h_i rows of w_i * pxsz bytes, back to back (what xpng_load returns).  The
 *                 images are reconstructed into a staging raster at the pitch of the widest image and copied out with a pitch per
 *                 image.  STAGING SIZE: the sum over the images of h_i * P bytes, P = (widest w) * pxsz rounded up to 16, each
 *                 image's share rounded up to 256; allocated by the first tight call, never shrunk, counted by
 *                 xpnghip_ctx_workspace_bytes.
 * nimg must equal the context's.  Every argument is checked before anything reaches the device: a rejected call writes nothing.
 * xpnghip_ctx_decode_status reports on the launch: a rejected tile leaves its own pixels undefined, every other tile of every
 * image is decoded. */
int xpnghip_decode_mixed_device_batch(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                      uint32_t nimg, const uint64_t *tile_off, void *const *d_outs, uint64_t out_bpr, void *stream);
/* Host buffers, one device (T and XPNG_GPUS do not apply): bodies[i] / lens[i] = file i's body after the 8-byte header,
 * dims = nimg pairs {w, h}, outs[i] = caller-allocated w_i * h_i * pxsz bytes, filled completely.  The sizes are walked on the
 * host; a truncated body or a rejected tile fails the whole call.  The images are decoded in the padded form and copied back row
 * by row, so the call needs device memory for the bodies, for sum of h_i rows at the widest image's pitch, and for the context
 * (about 8 bytes per pixel of the batch): size the batch accordingly (xpng_load_batch keeps a call under 2 GiB of padded rasters). */
int xpnghip_decode_mixed(int mode, int pxsz, uint32_t nimg, const uint8_t *const *bodies, const uint64_t *lens,
                         const uint64_t *dims, uint8_t *const *outs);

/* Encode every image of a mixed context in one launch sequence: the kernels of xpnghip_encode_device_batch, once over all M tiles
 * (the size-sorted work list where the uniform batch is tile-major; image after image where it is image-major).  One tile mode
 * per call: 1 (RGB and RGBA) or 2 (RGB only); an RGBA image narrower or shorter than 4 px is refused, as everywhere.  One
 * TRANSFORM FORM per call, as in a uniform batch: the strip kernels when no tile of the batch is wider than 672 px, the generic
 * kernel for all tiles otherwise (an image flatter or narrower than 444 px has such tiles); both give the same bytes.
 * nimg must equal the context's.
 *   in_bpr != 0  padded batch: d_rasters[i] (16-byte aligned) holds h_i rows at this one row pitch, >= (widest image) * pxsz, and
 *                has 16 readable bytes behind its last row (h_i * in_bpr + 16 bytes are always enough): the strip kernels fetch
 *                rows in aligned 16-byte pieces, as for a band (above).  The kernels read the caller's buffers directly; the bytes
 *                of a row past w_i * pxsz never influence the output.
 *   in_bpr == 0  tight rasters: d_rasters[i] holds h_i * w_i * pxsz bytes, rows back to back, at any alignment (what xpng_store
 *                is handed); nothing behind them is read.  A pack kernel copies them into the context's staging raster - the one
 *                of the tight decode, same size (STAGING SIZE above), allocated by the first tight call of either kind, counted by
 *                xpnghip_ctx_workspace_bytes - and the kernels read that.
 * d_blobs[i]: 4-byte aligned (a padded raster: 16-byte; the error text names the buffer and the alignment), capacity xpnghip_ctx_blob_bound(ctx, first_tile(i), first_tile(i + 1)); exactly the returned length
 * is written, nothing at or past the bound.  blobs_len, if not NULL, receives nimg lengths after one stream sync; with NULL read
 * xpnghip_ctx_last_blobs_len_at(ctx, i) after synchronising the stream yourself.
 * WORKSPACE: the first encode call allocates the encode workspace (about 4 or 5 B per pixel of the batch for the symbol planes,
 * 7.5 B per pixel + ~6 KB per tile of stream scratch - shared with the decode's planes, re-allocated once if a decode came first
 * and it is the larger: that one call waits for the context's earlier work and frees a buffer, which may make the runtime wait for
 * the whole device - and the per-tile tables, sized from M); mode 2 adds its own on first use.  All of it is counted by
 * xpnghip_ctx_workspace_bytes.  Every argument is checked before anything reaches the device: a rejected call writes nothing and
 * xpnghip_last_error() says why. */
int xpnghip_encode_varsize_device_batch(xpnghip_ctx *ctx, int mode, const void *const *d_rasters, uint64_t in_bpr,
                                        uint32_t nimg, void *const *d_blobs, uint64_t *blobs_len, void *stream);

/* ---- layouts: decode into and encode from planar, BGR and 3/4-channel device buffers (INTEGRATION.md "Layouts") ----------
 * The two calls above hand pixels over in the file's own form, interleaved R,G,B[,A].  The two below take a LAYOUT word for the
 * caller's buffers and do the rearrangement in the copy pass the tight forms already pay (the kernel that moves every image out of,
 * or into, the staging raster), so it costs no further pass over the pixels and no second copy of the batch. */
#define XPNGHIP_LAYOUT_PLANAR 0x001u  /* (C, H, W): plane c is h*w bytes at byte offset c*h*w, rows of w bytes back to back.
                                         Clear: interleaved (H, W, C), rows of w*C bytes back to back */
#define XPNGHIP_LAYOUT_BGR    0x002u  /* colour order B, G, R; alpha, when present, stays the last channel */
#define XPNGHIP_LAYOUT_C3     0x300u  /* bits 8..11 = channels C of the CALLER's buffers: 3 or 4; 0 = the context's pxsz */
#define XPNGHIP_LAYOUT_C4     0x400u
/* host-only: C (3 or 4) of a buffer of this layout on a context of `pxsz` bytes per pixel; -1 for unknown bits, a channel
 * field other than 0/3/4, or pxsz other than 3/4 */
int xpnghip_layout_channels(uint32_t layout, int pxsz);
/* Buffers in a layout are always TIGHT: image i is exactly C * w_i * h_i bytes at any alignment; nothing before or behind them is
 * read or written (there is no pitch).  The layout is checked with the other arguments before anything reaches the device: a
 * rejected call writes nothing and xpnghip_last_error() names the layout.
 *
 * Decode: xpnghip_decode_mixed_device_batch with out_bpr == 0 in everything but the copy-out - same checks, blobs, size walk,
 * xpnghip_ctx_decode_status and staging raster (STAGING SIZE above; no second buffer).  C == pxsz passes the channels through;
 * C == 4 on an RGB context writes alpha 255; C == 3 on an RGBA context drops alpha (the colours are the file's: a pixel of alpha 0
 * is 0,0,0, as the format stores it).  Layout 0 gives byte for byte what the tight form gives (it IS the tight form). */
int xpnghip_decode_varsize_device_batch_as(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                           uint32_t nimg, const uint64_t *tile_off, void *const *d_outs, uint32_t layout, void *stream);
/* Encode: xpnghip_encode_varsize_device_batch with in_bpr == 0 in everything but the pack-in.  C must equal the context's pxsz - a
 * lossless encoder does not drop or invent a channel - and a mismatch is refused with both numbers in the text.  The blobs are
 * byte for byte those of the tight-form encode of the equivalent interleaved R,G,B[,A] raster.  Of the caller's buffers only the
 * aligned dwords they occupy are read. */
int xpnghip_encode_varsize_device_batch_from(xpnghip_ctx *ctx, int mode, const void *const *d_rasters, uint32_t layout,
                                             uint32_t nimg, void *const *d_blobs, uint64_t *blobs_len, void *stream);

/* ---- float layouts: decode straight into normalised f16 / bf16 / f32 buffers -------------
 * A model reads floats, not the file's bytes.  The call below is xpnghip_decode_varsize_device_batch_as with one difference: the
 * copy-out pass converts while it rearranges, so the conversion costs no further pass over the pixels, no launch per image and no
 * intermediate uint8 buffer.  For every output element, with v the stored byte (0 .. 255) and c the channel's position in the
 * CALLER's buffer (after a BGR exchange, alpha last: with XPNGHIP_LAYOUT_BGR scale[0] belongs to blue):
 *     y   = fmaf((float)v, scale[c], bias[c])     one fp32 fused multiply-add, IEEE, subnormals kept
 *     out = (T)y                                  round to nearest even to T (f32: y itself); overflow of T gives +-inf
 * The alpha an RGB context does not store (C == 4 on pxsz == 3) is v = 255 through the same formula with c = 3; C == 3 on an RGBA
 * context drops alpha.  The dtype is an argument of its own, not a part of the layout word. */
#define XPNGHIP_DTYPE_F16  1u
#define XPNGHIP_DTYPE_BF16 2u
#define XPNGHIP_DTYPE_F32  3u
/* host-only: bytes of one element: 2, 2, 4; -1 for anything else (0 included: uint8 is not a dtype of the float call) */
int xpnghip_dtype_bytes(uint32_t dtype);
/* host-only, needs no device: the 256 outputs of channel position c for c = 0 .. C-1, i.e. table[c*256 + v] as an element of
 * `dtype`, computed with fmaf() and a round-to-nearest-even conversion on the host: bit for bit what the device call writes for the
 * byte v, so a caller that answers some images from host bytes stays consistent with it.  C = 1 .. 4.  -1 on a bad dtype, C, NULL,
 * or a non-finite scale / bias. */
int xpnghip_float_table(uint32_t dtype, int C, const float *scale, const float *bias, void *table);
/* scale and bias: C = xpnghip_layout_channels(layout, pxsz) floats each on the HOST, read during the call (they travel in the
 * kernel's arguments: no upload, no synchronisation); NULL scale = all ones, NULL bias = all zeros; every value must be finite.
 * Image i's buffer is TIGHT: C * w_i * h_i elements in the layout's order, aligned to the element size (2 or 4 bytes); exactly
 * C * w_i * h_i * sizeof(T) bytes are written and nothing before or behind them.  Same checks, blobs, size walk,
 * xpnghip_ctx_decode_status and staging raster as the layout call (no second buffer; the workspace grows by one record table).
 * Refused before anything reaches the device, with the offending value in xpnghip_last_error() and nothing written: a bad layout
 * word, a dtype outside 1 .. 3 (uint8 buffers are written by xpnghip_decode_varsize_device_batch_as), a non-finite constant, a
 * misaligned or NULL buffer, a context that is not mixed, a NULL context. */
int xpnghip_decode_varsize_device_batch_as_float(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                                 uint32_t nimg, const uint64_t *tile_off, void *const *d_outs, uint32_t layout,
                                                 uint32_t dtype, const float *scale, const float *bias, void *stream);

/* ---- crop, resize and flip in the same pass -------------------------------------------------
 * The float call above up to the copy-out - the same checks, blobs, size walk, staging raster and xpnghip_ctx_decode_status; every
 * tile is reconstructed as always - but the copy-out writes, for every image, a source rectangle resampled to ONE output size
 * out_h x out_w (each 1 .. 16384) with plain 2 x 2-tap bilinear interpolation (half-pixel centres, no antialiasing: for that see
 * xpnghip_decode_varsize_device_batch_resampled below), optionally
 * mirrored left to right.  Image i has the rectangle {x, y, w, h} = rects[4i .. 4i+3] (valid as for the region decode: not empty,
 * inside the image; rects == NULL: every whole image) and the flip flips[i] (0 or 1; flips == NULL: none).  With
 *     kx = (float)rw / (float)out_w,  ky = (float)rh / (float)out_h           one IEEE fp32 division each, on the host
 * output column ox (rows alike with ky, rh and no flip), u = flip ? out_w - 1 - ox : ox, is
 *     sx = max(fmaf((float)u + 0.5f, kx, -0.5f), 0.0f)
 *     x0 = min((uint32_t)sx, rw - 1)     x1 = min(x0 + 1, rw - 1)     lx = sx - (float)x0
 * and with p00 p01 / p10 p11 the bytes at (y + y0|y1, x + x0|x1) as floats - the byte of channel position c chosen as in the float
 * call: BGR exchange, alpha last, the alpha an RGB context lacks is 255 -
 *     a = fmaf(lx, p01 - p00, p00)   b = fmaf(lx, p11 - p10, p10)   v = fmaf(ly, b - a, a)
 *     y = fmaf(v, scale[c], bias[c])   out = (T)y                   round to nearest even
 * Edges clamp to the RECTANGLE, not the image.  A rectangle of the output's size is a pure crop (lx == ly == 0), bit for bit the
 * slice of the float call's output; a flip is a mirror on the bits.
 * d_outs[i] is exactly C * out_h * out_w elements in the layout's order, aligned to the element size (slices of one
 * (N, C, out_h, out_w) tensor qualify); nothing else is written.  The rectangle table (32 bytes per image) is uploaded on every
 * call and never cached; for that upload the call synchronises `stream` once BEFORE it queues its own kernels (the records are in
 * pageable host memory that ends with the call), so it waits for the caller's earlier work on the stream, never for its own.
 * Refused before anything reaches the device, with the offending value in xpnghip_last_error() and nothing written: a rectangle
 * that is empty or leaves its image (the text names the image), out_w or out_h outside 1 .. 16384, a flip byte other than 0 or 1,
 * and everything the float call refuses.  A rejected tile leaves the output elements with a tap inside it undefined; every other
 * element is written. */
int xpnghip_decode_varsize_device_batch_resized(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                                uint32_t nimg, const uint64_t *tile_off, void *const *d_outs, uint32_t layout,
                                                uint32_t dtype, const float *scale, const float *bias, const uint64_t *rects,
                                                const uint8_t *flips, uint32_t out_w, uint32_t out_h, void *stream);
/* host-only, needs no device: the same rule, bit for bit, applied to a tight interleaved host raster of h rows of w * pxsz bytes
 * (pxsz 3 or 4; w, h <= 1 << 24).  rect: {x, y, w, h} or NULL for the whole raster; flip 0 or 1; out: C * out_h * out_w elements
 * of `dtype` in `layout`, aligned to the element size.  What xpnghip_float_table is to the float call: for a caller that answers
 * some images without the codec.  0 on success; non-zero, with the offending value in xpnghip_last_error() and nothing written, on
 * a bad pxsz, layout, dtype, size, rectangle or flip, a non-finite constant, a NULL raster, or a NULL or misaligned out. */
int xpnghip_resize_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w,
                        uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias, void *out);

/* ---- the same pass with an antialiased downscale ----------------------------------------------
 * The resized call above with one more word, `filter`: */
#define XPNGHIP_FILTER_BILINEAR 0u    /* today's rule: exactly the resized call, the same kernel, the same bytes */
#define XPNGHIP_FILTER_TRIANGLE_AA 1u /* a triangle filter wherever an axis shrinks (what F.interpolate(antialias=True) computes) */
/* The rule of XPNGHIP_FILTER_TRIANGLE_AA.  Everything the host computes per image for the resized call stays:
 * kx = (float)rw / (float)OW and ky are computed on the host, one fp32 division each.  The record gains ikx = 1.0f / kx and
 * iky = 1.0f / ky, also one host fp32 division each.  The inverses travel in the per-image record.
 * An axis operation maps a sequence q(0 .. n-1) of fp32 values to one fp32 value.  Here n is the extent of the RECTANGLE on that
 * axis, O is the output extent and k is the ratio.  For output index u, the existing line f = fmaf((float)u + 0.5f, k, -0.5f) is
 * kept.
 *   k <= 1.0f, or filter 0.  Today's two taps, unchanged:
 *     s = max(f, 0)   i0 = min((uint32_t)s, n-1)   i1 = min(i0+1, n-1)   l = s - (float)i0
 *     result fmaf(l, q(i1) - q(i0), q(i0))
 *   k > 1.0f with filter 1.  A triangle of half-width k, clamped to the rectangle and renormalised:
 *     lo = f - k   j0 = lo > 0 ? (uint32_t)lo : 0   j1 = min((uint32_t)(f + k), n - 1)
 *     W = 0, A = 0, then for j = j0 .. j1 ascending:
 *         d = fabsf((float)j - f)   w = max(fmaf(-d, ik, 1.0f), 0.0f)   W = W + w   A = fmaf(w, q(j), A)
 *     result A / W, one IEEE fp32 division.
 * H(s) is the x-axis operation over the channel's bytes of source row s as floats, u = flip ? OW-1-ox : ox, as now.  v is the
 * y-axis operation over H(.).  Then, as now, y = fmaf(v, scale[c], bias[c]) and out = (T)y, round to nearest even.  Each axis
 * chooses its branch on its own k: a crop that shrinks in one direction and grows in the other mixes the branches.  Channel
 * choice, the BGR exchange, alpha last, the alpha an RGB context lacks (v = 255 exactly, no read), the constants, the layouts and
 * the dtypes are all as in the float and resized calls.
 * Consequences: (a) with filter 1, an image whose kx <= 1 and ky <= 1 gives bit for bit what filter 0 gives (the identity crop is
 * a special case); (b) a flip is a mirror on the bits; (c) no tap leaves the rectangle: the window is clamped to it, not to the
 * image.  W > 0 always.  Every multiplication is inside an explicit fmaf, sums and the division are single
 * operations, and the order of accumulation - ascending j within a row, ascending s over rows - is part of the rule.
 * The call takes the resized call's arguments plus `filter` and refuses what that call refuses; any filter other than 0 or 1 is
 * refused before anything reaches the device, with the value in xpnghip_last_error().  With filter 1 the per-image table is 48
 * bytes per image, uploaded on every call by the resized call's protocol. */
int xpnghip_decode_varsize_device_batch_resampled(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                                  uint32_t nimg, const uint64_t *tile_off, void *const *d_outs, uint32_t layout,
                                                  uint32_t dtype, const float *scale, const float *bias, const uint64_t *rects,
                                                  const uint8_t *flips, uint32_t out_w, uint32_t out_h, uint32_t filter, void *stream);
/* host-only, needs no device: the twin of the call above, bit for bit what it writes, as xpnghip_resize_host is of the resized
 * call (filter 0 IS xpnghip_resize_host).  Refuses a filter other than 0 or 1 and everything xpnghip_resize_host refuses, with
 * nothing written. */
int xpnghip_resample_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w,
                          uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter,
                          void *out);

/* ---- several views per image, only the tiles they touch --------------------------------------
 * The resampled call above writes one output per image, all of one size, and reconstructs every tile whatever the rectangles.  The
 * views call writes `nviews` outputs (1 .. 65535) from the `nimg` images of a mixed context - any number per image, none included -
 * each with its own rectangle, flip and output size, and decodes ONLY the tiles that some view of their image touches.
 *   view_image[v]   the image view v reads, 0 .. nimg-1.  NULL: the identity, and then nviews must equal nimg.
 *   rects           nviews * 4 values {x, y, w, h}, each valid inside ITS image as for the region decode.  NULL: whole images.
 *   flips           nviews bytes, 0 or 1.  NULL: none.
 *   out_sizes       nviews pairs {out_w, out_h}, each value 1 .. 16384; the sizes of one call may differ.  Required.
 *   d_outs[v]       exactly C * out_h_v * out_w_v elements of `dtype` in `layout`, aligned to the element size (slices of stacked
 *                   tensors qualify); nothing else is written.  Outputs that overlap are the caller's business.
 *   layout, dtype, scale, bias, filter   the resampled call's, one value per call.
 * THE VALUES.  View v of image i receives, bit for bit, what
 *     xpnghip_resample_host(pxsz, raster_i, w_i, h_i, rect_v, flip_v, out_w_v, out_h_v, layout, dtype, scale, bias, filter, out)
 * writes: that function is the rule, and consequences (a), (b) and (c) of the resampled call hold per view.
 * THE SELECTION.  A tile of the concatenated table is decoded if and only if it intersects the rectangle of at least one view of
 * its image (the test of xpnghip_region_tiles).  The launch list is the context's size-sorted list with the unselected entries
 * removed: decreasing pixel count, equal sizes in table order.  xpnghip_view_tiles below returns exactly that list, and the device
 * call uses the same function.  The size walk still covers every tile of every image (offsets are a serial sum), and the staging
 * raster, its slots and its size are those of every tight call (STAGING SIZE above).  Pixels of unselected tiles in the staging
 * raster are whatever earlier calls left; no tap reads them, because every window is clamped to its rectangle (consequence (c)).
 * xpnghip_ctx_decode_status reports on the tiles that were decoded: an unselected tile is not validated.
 * RECORDS.  One 64-byte record per view (the image's staging slot, the buffer, the rectangle, the output size, kx, ky, 1/kx, 1/ky
 * - one host fp32 division each, as in the resized and resampled calls - and the flip) and the selected list (4 bytes per tile)
 * are uploaded on every call and never cached, by the resized call's protocol: one upload and one synchronisation of `stream`,
 * queued before the call's own kernels.  Both buffers belong to the context's workspace and grow only when a call needs more than
 * any call before it.  The cached per-image table of the other tight calls is not touched.
 * Refused before anything reaches the device, with the offending value in xpnghip_last_error() and nothing written: nviews outside
 * 1 .. 65535; NULL view_image with nviews != nimg; a view_image[v] >= nimg (the text names the view); an invalid rectangle (the
 * view and the image); an output size outside 1 .. 16384 (the view); a flip byte above 1; a filter other than 0 or 1; NULL
 * out_sizes; a NULL or misaligned d_outs[v]; and everything the float call refuses. */
int xpnghip_decode_varsize_device_batch_views(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                              uint32_t nimg, const uint64_t *tile_off, uint32_t nviews, const uint32_t *view_image,
                                              void *const *d_outs, const uint32_t *out_sizes, const uint64_t *rects,
                                              const uint8_t *flips, uint32_t layout, uint32_t dtype, const float *scale,
                                              const float *bias, uint32_t filter, void *stream);
/* host-only, needs no device: the launch list of a views call over images of `dims` (nimg pairs {w, h}, as for
 * xpnghip_ctx_create_mixed) - indices into the concatenated tile table, in launch order.  view_image and rects as above (NULL
 * allowed as above).  Returns the count, or -1 on a bad argument or when `cap` entries are too few. */
int64_t xpnghip_view_tiles(const uint64_t *dims, uint32_t nimg, uint32_t nviews, const uint32_t *view_image, const uint64_t *rects,
                           uint32_t *tiles, uint64_t cap);
/* The number of tile work items in the context's most recent decode launch: M after the other mixed calls, the length of the list
 * after a views or a region call, nimg * (t1 - t0) after a range decode, 0 before any decode. */
uint64_t xpnghip_ctx_last_decode_tiles(const xpnghip_ctx *ctx);

/* ---- a colour matrix per view in the copy-out of a views call -------------------------------
 * Two-view and multi-crop pipelines give every view a colour jitter of its own, and some views a grayscale.  Brightness, contrast
 * about a fixed centre, saturation, a hue rotation, grayscale, a channel permutation and every product of them are linear per
 * pixel: one 3 x 4 matrix.  The copy-out pass holds every output value in a register just before the store, so the matrix is
 * applied there and no further pass over the views is needed.
 * THE RULE.  `colour` is 12 floats, row-major 3 x 4.  Row k is the OUTPUT colour k in the order R, G, B - whatever the layout's BGR
 * bit says - and the columns are the inputs R, G, B and a constant, all in byte units (0 .. 255).  With vR, vG, vB the fp32 values
 * the resample rule above produces for the three colour bytes of an output pixel (its v, before the constants):
 *     t_k = fmaf(m[k][0], vR, fmaf(m[k][1], vG, fmaf(m[k][2], vB, m[k][3])))      three explicit fp32 fmas, this nesting
 *     t_k = t_k < 0.0f ? 0.0f : t_k > 255.0f ? 255.0f : t_k                       the clamp a uint8 pipeline would apply
 *     y   = fmaf(t_k, scale[c], bias[c])    out = (T)y                            as above; c = position in the CALLER's buffer
 * With XPNGHIP_LAYOUT_BGR position c < 3 holds colour k = 2 - c.  Alpha does not pass through the matrix: position 3, whether it
 * is stored or the 255 an RGB context lacks, takes fmaf(v, scale[3], bias[3]) as above, and C == 3 on an RGBA context drops alpha
 * as above.  Every entry must be finite with |m| <= 65536, so that no intermediate overflows and no NaN can arise; anything else
 * is refused before anything is written, and the message names the entry (and, in the device call, the view).
 * Consequences: (d) with filter 0 an identity matrix gives bit for bit what colour == NULL gives, because every v lies within
 * 0 .. 255 and fmaf(1, v, 0 + 0) is v; with filter 1 the quotient A / W may round a hair past 255 and the clamp may then differ,
 * which is why NULL, not the identity, is the "off" value; (e) a flip is still a mirror on the bits; (f) no tap leaves the
 * rectangle: nothing about the source side changes.
 * host-only, needs no device: xpnghip_resample_host with one more argument.  colour == NULL is xpnghip_resample_host itself. */
int xpnghip_resample_colour_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip,
                                 uint32_t out_w, uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale,
                                 const float *bias, uint32_t filter, const float *colour, void *out);
/* The views call with `colours`: nviews * 12 floats on the host, the matrix of view v at colours + 12 * v.  View v receives, bit
 * for bit, what xpnghip_resample_colour_host writes with its matrix.  colours == NULL is the views call: the same kernel, the same
 * bytes, and nothing more allocated or uploaded.  The checks, their order and their texts are the views call's, followed by the
 * matrices' (the text names the view and the entry).  The matrices travel in a table of their own, 48 bytes per view, which belongs
 * to the context's workspace, grows only when a call has more views than any colour call before it, and is uploaded with the
 * views call's two tables in front of the call's kernels, under the same single synchronisation of `stream`.  The 64-byte view
 * record, the selection and the decode stages are the views call's. */
int xpnghip_decode_varsize_device_batch_views_colour(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                                     uint32_t nimg, const uint64_t *tile_off, uint32_t nviews,
                                                     const uint32_t *view_image, void *const *d_outs, const uint32_t *out_sizes,
                                                     const uint64_t *rects, const uint8_t *flips, uint32_t layout, uint32_t dtype,
                                                     const float *scale, const float *bias, uint32_t filter, const float *colours,
                                                     void *stream);

/* ---- antialiased bicubic resampling in the copy-out of a views call -------------------------
 * DINO, BYOL, MAE and the ViT recipes resize with BICUBIC: PIL's BICUBIC, F.interpolate(mode="bicubic", antialias=True) on tensors.
 * Every entry point above that takes a `filter` word keeps its domain, 0 or 1.  The cubic rule has entry points of its own, which
 * take no filter word at all: they are always this rule.
 * THE RULE.  Everything outside the axis operation is the views-colour call's: the 64-byte view record (nothing added), the
 * selection of tiles, channel choice, the BGR exchange, alpha last, the layouts, the dtypes and the constants; v = 255 exactly, with
 * no read, still stands in for the alpha an RGB context lacks.  One axis operation maps q(0 .. n-1), fp32, to one fp32 value; n is
 * the extent of the RECTANGLE on the axis, k the ratio from the record and ik its inverse, also from the record.  For output
 * index u:
 *     f  = fmaf((float)u + 0.5f, k, -0.5f)                  (as above)
 *     s  = k > 1.0f ? k : 1.0f       is = k > 1.0f ? ik : 1.0f       r = s + s
 *     lo = f - r    j0 = lo > 0 ? (uint32_t)lo : 0          j1 = min((uint32_t)(f + r), n - 1)
 *     W = 0, A = 0, then for j = j0 .. j1 ascending:
 *         d = fabsf((float)j - f)        t = fmaf(d, is, 0.0f)
 *         w = t < 1 ? fmaf(fmaf(fmaf( 1.5f, t, -2.5f), t,  0.0f), t, 1.0f)
 *           : t < 2 ? fmaf(fmaf(fmaf(-0.5f, t,  2.5f), t, -4.0f), t, 2.0f)
 *           : 0.0f
 *         W = W + w        A = fmaf(w, q(j), A)
 *     result A / W        one IEEE fp32 division
 * This is Keys' cubic with a = -0.5, stretched by the ratio where the axis shrinks, clamped to the rectangle and renormalised: the
 * kernel and the window of PIL's BICUBIC and of ATen's _upsample_bicubic2d_aa.  Unlike the triangle rule there is no two-tap
 * branch: an axis with k <= 1 takes the same window with s = 1, four to five taps.  H(s) is the x-axis operation over row s of the
 * rectangle with u = flip ? OW-1-ox : ox, and the y-axis operation runs over H(.).  Then
 *     v = result < 0.0f ? 0.0f : result > 255.0f ? 255.0f : result
 * because a cubic overshoots (random bytes range about -47 .. 272) and a uint8 pipeline clamps exactly there.  After that the colour
 * matrix applies where one is given, by the rule of the views-colour call on these clamped v; last y = fmaf(v_or_t, scale[c],
 * bias[c]) and out = (T)y, round to nearest even.  Every multiplication is inside an explicit fmaf, sums and the division are
 * single operations, and the order of accumulation - ascending j within a row, ascending s over rows - is part of the rule.
 * Consequences: (a) a rectangle of the output's size is a pure crop, bit for bit the slice of the float call: at k = 1, f is an
 * integer and the weights are exactly 1, 0, 0; (b) a flip is a mirror on the bits; (c) no tap leaves the rectangle, which is what
 * keeps skipping untouched tiles safe; (d) an identity matrix gives the bits of colour == NULL, because v already lies in
 * 0 .. 255 (under the triangle filter this does not hold).  W > 0 always.
 * host-only, needs no device, and it is the rule: the arguments of xpnghip_resample_colour_host without `filter`; colour may be
 * NULL.  Refuses everything xpnghip_resample_colour_host refuses, with the same texts and with nothing written. */
int xpnghip_resample_cubic_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip,
                                uint32_t out_w, uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale,
                                const float *bias, const float *colour, void *out);
/* The views-colour call without `filter`: view v receives, bit for bit, what xpnghip_resample_cubic_host writes with its matrix
 * (colours == NULL: with colour == NULL, and then no matrix table is allocated or uploaded).  The checks, their order and their
 * texts - without the filter's -, the selection (xpnghip_view_tiles), the records, the upload protocol, the workspace growth and
 * xpnghip_ctx_last_decode_tiles are the views-colour call's. */
int xpnghip_decode_varsize_device_batch_views_cubic(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                                    uint32_t nimg, const uint64_t *tile_off, uint32_t nviews,
                                                    const uint32_t *view_image, void *const *d_outs, const uint32_t *out_sizes,
                                                    const uint64_t *rects, const uint8_t *flips, uint32_t layout, uint32_t dtype,
                                                    const float *scale, const float *bias, const float *colours, void *stream);

/* ---- Gaussian blur and solarise per view in a views call ------------------------------------
 * SimCLR, BYOL and DINO put a Gaussian blur with a sigma per view, and a solarise on the second view, between the colour jitter
 * and the normalisation.  Neither is linear per pixel and a blur reads its neighbours' finished values, so views that ask for
 * either take a second pass.  One 16-byte record per view: */
typedef struct { float sigma; uint32_t radius; float solarise; uint32_t reserved; } xpnghip_view_blur;
/* radius is 0 .. 31: the blur has 2 * radius + 1 taps per axis.  0 means no blur, and then sigma must be 0.0f; with radius > 0,
 * sigma must be finite and lie in 2^-10 .. 1024.  solarise is a threshold in byte units: 0 .. 255 turns it on, exactly 256.0f turns
 * it off, anything else (NaN included) is refused.  reserved must be 0.  {0.0f, 0, 256.0f, 0} is the record that is all off.
 * The third filter word.  It is accepted ONLY by the two functions of this section, where it selects the rule of
 * xpnghip_resample_cubic_host; every other entry point with a filter word keeps its domain of 0 and 1. */
#define XPNGHIP_FILTER_CUBIC_AA 2u
/* THE WEIGHTS, host-only: w[0 .. radius] (radius + 1 floats) of the blur, one statement for the device call, the host rule, Python
 * and the tests.  In double: g[d] = exp(-(double)(d * d) / (2.0 * s * s)) with s = (double)sigma; S = g[0] + 2 * (g[1] + .. + g[R]),
 * the inner sum in ascending d; w[d] = (float)(g[d] / S).  Returns 1, with the text, for radius > 31, for a sigma that is not
 * finite or outside 2^-10 .. 1024 with radius > 0, for a sigma other than 0.0f with radius 0, and for w == NULL; radius 0 gives
 * w[0] = 1.0f.
 * THE RULE.  The intermediate T - C planes of out_h x out_w fp32 in byte units - is, bit for bit, what the existing host functions
 * write for the view: xpnghip_resample_colour_host for filter 0 or 1, xpnghip_resample_cubic_host for filter 2, with layout
 * XPNGHIP_LAYOUT_PLANAR | (C << 8) without the BGR bit, dtype F32, every scale 1.0f, every bias 0.0f and the view's matrix where
 * it has one.  Nothing about resampling or colour is restated here.  The blur applies to the three colour planes only: alpha, or
 * the 255 an RGB context lacks, passes through untouched, as with the colour matrix.  With
 *     refl(i, n) = i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i              (torch's "reflect")
 * the horizontal operation on plane q is, in fp32 with explicit fmaf,
 *     A = 0.0f
 *     for d = R down to 1:  A = fmaf(w[d], q(y, refl(x - d, out_w)) + q(y, refl(x + d, out_w)), A)
 *     A = fmaf(w[0], q(y, x), A)
 * and the vertical operation is the same over the horizontal results, with out_h.  Then b = A < 0 ? 0 : A > 255 ? 255 : A.  With
 * R == 0 the blur step is skipped and b = q.  The order of accumulation is part of the rule.  Solarise, where it is on:
 * b = b >= thr ? 255.0f - b : b, on the colour channels only.  Last y = fmaf(b, scale[c], bias[c]) and out = (T)y; the BGR exchange
 * and c, the position in the caller's buffer, are exactly the existing calls'.
 * Refused, before anything is written or reaches the device, with a text that names the view (in the device call) and the field:
 * radius > 31; radius >= out_w or radius >= out_h of that view (reflect needs it, and torch refuses the same); the sigma, solarise
 * and reserved conditions above; a filter above 2; everything the underlying call refuses.
 * Consequences: (a) a record that is all off gives the bits of the plain call for that view, and blurs == NULL IS the underlying
 * call: same kernels, same bytes, nothing more allocated or uploaded; (b) a flip is still a mirror on the bits, because the pair
 * sum commutes; (c) no tap leaves the view's own plane.
 * Not offered: PIL's ImageFilter.GaussianBlur (a box-blur approximation), blurred alpha, uint8 outputs.
 * host-only, needs no device, and it is the rule: xpnghip_resample_colour_host's arguments, with filter 0, 1 or 2, plus one record
 * (NULL: all off).  colour may be NULL. */
int xpnghip_blur_weights(float sigma, uint32_t radius, float *w);
int xpnghip_resample_blur_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip,
                               uint32_t out_w, uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale,
                               const float *bias, uint32_t filter, const float *colour, const xpnghip_view_blur *blur, void *out);
/* The views-colour call plus `blurs`: nviews records on the host, or NULL.  View v receives, bit for bit, what
 * xpnghip_resample_blur_host writes with its matrix and its record.  filter may be 0, 1 or 2; colours may be NULL.  Views whose
 * record is all off are written by the copy-out kernel of the underlying call, straight into the caller's buffer.  The others are
 * written by that kernel as fp32 planes into a scratch of the context's workspace - C * out_h * out_w floats per view, each slice
 * rounded up to 256 bytes; counted by xpnghip_ctx_workspace_bytes; it grows only when a call needs more than any call before it -
 * and a second kernel (xpng_amd/csrc/mixed_views_blur.hpp) blurs, solarises, applies the constants and stores.  The tables of the
 * second pass are uploaded with the call's other tables under the same single synchronisation. */
int xpnghip_decode_varsize_device_batch_views_blur(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                                   uint32_t nimg, const uint64_t *tile_off, uint32_t nviews,
                                                   const uint32_t *view_image, void *const *d_outs, const uint32_t *out_sizes,
                                                   const uint64_t *rects, const uint8_t *flips, uint32_t layout, uint32_t dtype,
                                                   const float *scale, const float *bias, uint32_t filter, const float *colours,
                                                   const xpnghip_view_blur *blurs, void *stream);

/* ---- an affine map per view in the copy-out of a views call ----------------------------------
 * RandomRotation, RandomAffine, the rotate / shear / translate operations of RandAugment, AutoAugment and TrivialAugment, and the
 * rotations of detection and segmentation pipelines with nearest-neighbour sampling for their label maps.  Every geometric
 * operation above is an axis-aligned rectangle with an optional mirror; here a view has an inverse 2 x 3 matrix instead, which
 * carries the crop, the size change, the mirror, the rotation and the shear at once, and one fill per call for what lies outside.
 * THE RULE.  `affine` is 6 floats, row-major 2 x 3, from continuous OUTPUT coordinates to continuous SOURCE coordinates of the
 * whole image; pixel (j, i) has its centre at (j + 0.5, i + 0.5).  For output pixel (ox, oy), X = (float)ox + 0.5f and
 * Y = (float)oy + 0.5f:
 *     sx = fmaf(m[0], X, fmaf(m[1], Y, m[2])) - 0.5f        this nesting; the subtraction is one fp32 operation
 *     sy = fmaf(m[3], X, fmaf(m[4], Y, m[5])) - 0.5f
 * THE FOOTPRINT F of a view, computed on the host in double from the fp32 entries: the source coordinates of the four corner output
 * pixels (ox in {0, out_w-1}, oy in {0, out_h-1}; the map is affine, so the extremes are there),
 *     F = [floor(min sx) - 1, floor(max sx) + 2] x [floor(min sy) - 1, floor(max sy) + 2]   intersected with the image; it may be empty.
 * A TAP q(j, i, c) is the image's byte as fp32 where (j, i) lies inside F, and fill[k] everywhere else, k the colour R, G, B or A
 * of that channel.  `fill` is 4 floats in byte units, each finite and within 0 .. 255; NULL means zeros.  The test is made on the
 * integer tap, so no tap leaves F by construction; and F contains every tap that exact arithmetic would place inside the image,
 * because the entry bounds below keep the fp32 error of sx and sy below 0.1 against F's margin of one whole pixel.  The alpha an
 * RGB context lacks is still v = 255 exactly, with no read.
 *     filter XPNGHIP_FILTER_BILINEAR (0)    x0 = floorf(sx)  lx = sx - x0    y0 = floorf(sy)  ly = sy - y0
 *         t = fmaf(lx, q(x0+1, y0)   - q(x0, y0),   q(x0, y0))
 *         u = fmaf(lx, q(x0+1, y0+1) - q(x0, y0+1), q(x0, y0+1))
 *         v = fmaf(ly, u - t, t)
 *       which is torchvision's tensor affine() with `fill`, i.e. grid_sample(padding_mode="zeros", align_corners=False) blended
 *       with a mask;
 *     filter XPNGHIP_FILTER_NEAREST (3)     v = q((int)rintf(sx), (int)rintf(sy)), ties to even: grid_sample's rule.
 * The fourth filter word is accepted ONLY by the functions of this section, and they accept 0 and 3 only. */
#define XPNGHIP_FILTER_NEAREST 3u
/* Behind v everything is the views-colour rule, unchanged: the optional 3 x 4 matrix and its clamp, y = fmaf(v_or_t, scale[c],
 * bias[c]), out = (T)y, the BGR exchange, alpha last, the layouts and the dtypes.
 * ENTRY BOUNDS.  Every entry finite, and |m[0]| * out_w, |m[1]| * out_h, |m[2]| (and the same of the second row) each at most
 * 2^18 = 262144.  Every source coordinate of the view and every intermediate of the rule then stays below 2^20 in magnitude -
 * inside the 2^22 at which a view must be refused -, an fp32 operation there errs by at most 2^-5, and three of them by less than
 * 0.1 of a pixel.  Anything else is refused before anything is written; the text names the entry (and, in the device call, the view).
 * Consequences: (a) the matrix {1, 0, x, 0, 1, y} with integer x, y and the view inside the image is a pure crop, bit for bit the
 * slice of the float call, under both filters: sx is an integer, lx = 0 and fmaf(0, d, q) = q; (b) an exact quarter turn - entries
 * 0 and +-1, constants integers or half-integers that put sx, sy on integers - is bit for bit np.rot90 of the crop, and the mirror
 * matrix {-1, 0, x + w, 0, 1, y} gives the bits of the flip; (c) no tap leaves F; (d) a view whose F is empty is all fill, then
 * the matrix and the constants, and it selects no tile.
 * Not offered: antialiasing under a shrinking map (torchvision has none either); bicubic under a warp; blur or solarise in the same
 * call; perspective maps; uint8 outputs; a fill per view.
 * host-only, needs no device: the footprint of one view over a w x h image as rect = {x, y, w, h} ({0, 0, 0, 0}: empty).  Returns 1,
 * with the text, for a bad image size, output size or matrix. */
int xpnghip_affine_footprint(uint64_t w, uint64_t h, const float *affine, uint32_t out_w, uint32_t out_h, uint64_t *rect);
/* host-only, needs no device, and it is the rule.  No rect and no flip: the matrix carries both.  filter is 0 or 3; fill and colour
 * may be NULL.  Refuses, in this order and with nothing written: the filter; everything xpnghip_resample_colour_host refuses of its
 * other arguments, with the same texts; the matrix; the fill; the colour matrix. */
int xpnghip_resample_affine_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const float *affine, uint32_t out_w,
                                 uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias,
                                 uint32_t filter, const float *fill, const float *colour, void *out);
/* host-only, needs no device: the launch list of an affine views call, the sibling of xpnghip_view_tiles.  affines is nviews * 6
 * floats, out_sizes nviews pairs.  A tile is listed if and only if it intersects the footprint of at least one view of its image
 * (region_select's test on the footprints; an empty footprint selects nothing); the order is xpnghip_view_tiles'.  Returns the
 * count, or -1 on a bad argument or when `cap` entries are too few.  The device call uses the same function. */
int64_t xpnghip_affine_view_tiles(const uint64_t *dims, uint32_t nimg, uint32_t nviews, const uint32_t *view_image,
                                  const float *affines, const uint32_t *out_sizes, uint32_t *tiles, uint64_t cap);
/* The views-colour call with `affines` (nviews * 6 floats on the host, required) and `fill` (4 floats on the host, or NULL) in
 * place of rects and flips.  View v of image i receives, bit for bit, what xpnghip_resample_affine_host writes for raster_i with its
 * matrix, the call's fill and, where colours is given, its colour matrix.  The checks, their order and their texts are the
 * views-colour call's, with the rectangles' and the flips' replaced by the fill's (once per call, in front of the views) and the
 * matrices' (per view, where the rectangle's stood); the filter must be 0 or 3.  Nothing is written when a call is refused.
 * SELECTION: xpnghip_affine_view_tiles.  RECORDS: one 64-byte record per view (the staging slot, the buffer, the six floats, out_w,
 * out_h and the footprint) in a table of its own in the context's workspace - counted by xpnghip_ctx_workspace_bytes, grown only
 * when a call has more views than any affine call before it - uploaded with the selected list and, where given, the colour table
 * under the views call's single synchronisation.  The views call's own record table is neither used nor allocated.  The fill
 * travels in the kernel's arguments.  One kernel, xpng_amd/csrc/mixed_views_affine.hpp, writes every view.  A call whose views ALL
 * have an empty footprint decodes nothing - xpnghip_ctx_last_decode_tiles is 0 and the status is clear - and writes the fill. */
int xpnghip_decode_varsize_device_batch_views_affine(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                                     uint32_t nimg, const uint64_t *tile_off, uint32_t nviews,
                                                     const uint32_t *view_image, void *const *d_outs, const uint32_t *out_sizes,
                                                     const float *affines /* nviews * 6 */, const float *fill, uint32_t layout,
                                                     uint32_t dtype, const float *scale, const float *bias, uint32_t filter,
                                                     const float *colours, void *stream);

/* ---- autocontrast, equalise, posterise, solarise and invert per view -------------------------
 * The tone operations of AutoAugment, RandAugment and TrivialAugment, in any order, behind the blur call or the affine call.
 * Autocontrast and equalise need a statistic over the whole finished plane, so a view with a step takes a second pass.  One
 * 20-byte TONE RECORD per view, up to four steps executed in order: */
typedef struct { uint8_t op[4]; float arg[4]; } xpnghip_view_tone;   /* 20 bytes */
#define XPNGHIP_TONE_NONE 0u          /* arg 0 */
#define XPNGHIP_TONE_AUTOCONTRAST 1u  /* arg 0 */
#define XPNGHIP_TONE_EQUALISE 2u      /* arg 0 */
#define XPNGHIP_TONE_POSTERISE 3u     /* arg = bits, an integer 0 .. 8 */
#define XPNGHIP_TONE_SOLARISE 4u      /* arg = threshold, 0 .. 255 */
#define XPNGHIP_TONE_INVERT 5u        /* arg 0 */
/* Steps are contiguous from index 0: after the first NONE every later op is NONE.
 * THE RULE.  The steps run on the three colour planes - alpha, or the 255 an RGB context lacks, passes through untouched - on
 * exactly the values q the underlying call would hand to scale / bias: after resampling, colour matrix, blur and its clamp and the
 * blur record's own solarise; before the constants, the BGR exchange and the narrowing.  Per colour plane, N = out_h * out_w:
 *     entry          b = q > 0.0f ? (q > 255.0f ? 255.0f : q) : 0.0f
 *                    (a clamp that also maps -0.0f to +0.0f: every later value is a non-negative float in 0 .. 255)
 *     autocontrast   lo, hi = the minimum and maximum of the plane as the earlier steps left it.  hi == lo: unchanged.  Otherwise
 *                    s = 255.0f / (hi - lo), an fp32 subtraction and a correctly rounded fp32 division; where s is infinite
 *                    (hi - lo below about 7.5e-37) the plane is unchanged too; t = (b - lo) * s, an fp32
 *                    subtraction and an fp32 multiplication, never fused; b = t > 255.0f ? 255.0f : t
 *                    (torchvision's autocontrast on a float tensor, in byte units)
 *     equalise       n = (uint32_t)rintf(b), ties to even, 0 .. 255; h[n] the count of n over the plane; last = the highest non-empty
 *                    bin; step = (N - h[last]) / 255 in integers.  step == 0: unchanged (fractional values stay fractional).
 *                    Otherwise b = (float)min(255, (step / 2 + h[0] + .. + h[n - 1]) / step), integer division
 *                    (on integer-valued planes PIL's ImageOps.equalize and torchvision's equalize, value for value)
 *     posterise k    m = 2^(8 - k); b = b - fmodf(b, m), exact in fp32.  k = 8 floors a fractional value, k = 0 gives 0
 *                    (on integer values b & mask: ImageOps.posterize)
 *     solarise thr   b = b >= thr ? 255.0f - b : b
 *     invert         b = 255.0f - b
 * A step's statistics are taken over the plane as all earlier steps left it.  Minimum, maximum and integer counts do not depend on
 * the order in which a plane is reduced, so the device calls below equal the host functions bit for bit.
 * Refused, before anything is written or reaches the device, with a text that names the view (in the device calls) and the step:
 * an op above 5; a non-NONE op after a NONE; a non-zero arg on an op that takes none; posterise bits that are not an integer in
 * 0 .. 8; a threshold that is not finite or lies outside 0 .. 255; everything the underlying call refuses.
 * Not offered: sharpness (a stencil: it belongs with the blur); torchvision's contrast about the image's own mean (a float mean
 * depends on the order of summation); blur under a warp; more than four steps; uint8 outputs.
 * host-only, need no device, and they are the rule: xpnghip_resample_blur_host's and xpnghip_resample_affine_host's arguments plus
 * one tone record (NULL: no step, the underlying function's bits). */
int xpnghip_resample_tone_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip,
                               uint32_t out_w, uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale,
                               const float *bias, uint32_t filter, const float *colour, const xpnghip_view_blur *blur,
                               const xpnghip_view_tone *tone, void *out);
int xpnghip_resample_affine_tone_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const float *affine, uint32_t out_w,
                                      uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias,
                                      uint32_t filter, const float *fill, const float *colour, const xpnghip_view_tone *tone,
                                      void *out);
/* The blur call and the affine call with `tones` (nviews records on the host, or NULL) in front of `stream`.  View v receives, bit
 * for bit, what the host function above writes with its record.  tones == NULL, or records that are all NONE, IS the underlying
 * call: same kernels, same bytes, nothing more allocated or uploaded.  In the blur form blurs and colours may be NULL and filter is
 * 0, 1 or 2; in the affine form filter is 0 or 3, the fill pixels take part in the statistics, and blur under a warp stays not
 * offered.  A view with a step is a second-pass view: the copy-out kernel of the call writes its fp32 planes into the scratch of the
 * blur call (a second slice of the same size where the view also blurs); per step index one statistics launch (only where some
 * view's step there is autocontrast or equalise) and one apply launch rewrite the planes in place
 * (xpng_amd/csrc/mixed_views_tone.hpp); the blur call's second kernel, with a record that is all off, writes the caller's buffer.
 * The workspace gains one 48-byte record per tone view and one statistics slot of 3096 bytes per (tone view, statistics step),
 * zeroed on the stream by every call, both counted by xpnghip_ctx_workspace_bytes and grown only when a call needs more than any
 * call before it. */
int xpnghip_decode_varsize_device_batch_views_tone(xpnghip_ctx *ctx, int mode, const void *const *d_blobs, const uint64_t *blobs_len,
                                                   uint32_t nimg, const uint64_t *tile_off, uint32_t nviews,
                                                   const uint32_t *view_image, void *const *d_outs, const uint32_t *out_sizes,
                                                   const uint64_t *rects, const uint8_t *flips, uint32_t layout, uint32_t dtype,
                                                   const float *scale, const float *bias, uint32_t filter, const float *colours,
                                                   const xpnghip_view_blur *blurs, const xpnghip_view_tone *tones, void *stream);
int xpnghip_decode_varsize_device_batch_views_affine_tone(xpnghip_ctx *ctx, int mode, const void *const *d_blobs,
                                                          const uint64_t *blobs_len, uint32_t nimg, const uint64_t *tile_off,
                                                          uint32_t nviews, const uint32_t *view_image, void *const *d_outs,
                                                          const uint32_t *out_sizes, const float *affines /* nviews * 6 */,
                                                          const float *fill, uint32_t layout, uint32_t dtype, const float *scale,
                                                          const float *bias, uint32_t filter, const float *colours,
                                                          const xpnghip_view_tone *tones, void *stream);

/* ---- staged batch from device tensors: the inverse of the float call --------------------------
 * A model writes floats, not the file's bytes.  The call below is xpnghip_images_begin with the upload replaced by one staging
 * kernel that reads the caller's DEVICE buffers - planar or interleaved, RGB or BGR, uint8, f16, bf16 or f32 - and writes the
 * interleaved R,G,B[,A] bytes of the staged rasters, so model outputs reach .xpng files without crossing to the host and back and
 * without a torch op per image.  For every element x of a buffer - f16 or bf16 widened exactly to fp32 (subnormals kept), f32 as it
 * is - and c the channel's position in the CALLER's buffer (with XPNGHIP_LAYOUT_BGR scale[0] belongs to blue; alpha is always
 * last: the float call's convention):
 *     y = fmaf(x, scale[c], bias[c])      one fp32 fused multiply-add, IEEE, subnormals kept, a value of its own
 *     v = 0      if y is NaN or y <= 0    (-0 and -inf included)
 *         255    if y >= 255              (+inf included)
 *         (uint8_t)rintf(y) otherwise     round half to even: 0.5 -> 0, 1.5 -> 2, 254.5 -> 254
 * dtype 0 means the buffer already holds uint8: v = x, and scale and bias must both be NULL (the call is refused otherwise).
 *
 * d_bufs[i] is TIGHT: channels[i] * w_i * h_i elements of `dtype` (dims = nimg pairs {w, h}; channels[i] = 3 or 4, per image) in
 * the layout's order, aligned to the element size; of a buffer only the aligned dwords it occupies are read.  `layout` carries the
 * PLANAR and BGR bits only: a channel field other than 0 is refused, the count is per image.  scale and bias: four floats each on
 * the HOST (they travel in the kernel's arguments), NULL = all ones / all zeros, every value finite.  The staging kernel is queued
 * on `stream` (a stream of `device`, or NULL), so it runs behind whatever produced the buffers there; the handle's own stream
 * waits for it through an event, and normalize_RGBA and the one read-back of the flags follow as in xpnghip_images_begin.  When
 * the call returns the caller's buffers are free again, pxsz_out[i] = bytes per pixel of the normalised raster, and every other
 * xpnghip_images_* call works on the handle unchanged.  The handle lives on `device` (XPNG_DEVICE does not apply).
 * Refused before anything reaches the device, with the offending value in xpnghip_last_error() and *h == NULL: a NULL or
 * misaligned buffer, a side outside 1 .. 1 << 24, a channel count other than 3 or 4, a bad layout word or dtype, constants with
 * dtype 0, a non-finite constant, nimg outside 1 .. 4096, no such device. */
int xpnghip_images_begin_device(xpnghip_images **h, int device, uint32_t nimg, const void *const *d_bufs, const uint64_t *dims,
                                const uint8_t *channels, uint32_t layout, uint32_t dtype, const float *scale, const float *bias,
                                void *stream, uint8_t *pxsz_out);
/* host-only, needs no device: the same rule, bit for bit, applied to a tight HOST buffer of C * npx elements (C = 3 or 4) in
 * `layout` (PLANAR and BGR bits only); out receives npx * C interleaved R,G,B[,A] bytes.  For a caller that answers some images on
 * the host.  0 on success; non-zero, with the offending value in xpnghip_last_error() and nothing written, on a bad layout, dtype
 * or C, constants with dtype 0, a non-finite constant, or a NULL buffer. */
int xpnghip_quantize_host(uint32_t layout, uint32_t dtype, int C, const void *src, uint64_t npx, const float *scale,
                          const float *bias, uint8_t *out);

/* Stage-only run for BASELINE config 2: predictor chooser + per-pixel transform (libxpng.c:92-140 and
 * the arithmetic of 497-519) over tiles [t0, t1); symbol planes stay in the context's workspace. */
int xpnghip_m1_transform_device(xpnghip_ctx *ctx, const void *d_raster, uint64_t t0, uint64_t t1, void *stream);
int xpnghip_m1_transform_device_batch(xpnghip_ctx *ctx, const void *const *d_rasters, uint32_t nimg, uint64_t t0,
                                      uint64_t t1, void *stream);

/* ---- introspection for parity tests (copies intermediates of the LAST encode to host) --------------
 * what: 0 = predictor byte pr (1 B), 1..5 = planes nl,r,g,b,a (w*h B each, tile-linear),
 *       10..18 = context stream 0..8, 19 = residual bit-stream words k, 20..29 = rANS block 0..9,
 *       30 = chooser cost sums (16 B).  Returns bytes written to `out` (<= cap) or -1. */
int64_t xpnghip_debug_fetch(xpnghip_ctx *ctx, int what, uint64_t tile, void *out, uint64_t cap);

/* ---- wave probe for placement studies (tools/wave_probe.py; no reference counterpart) ---------------
 * Exists only in libxpng_hip_probes.so (xpnghip_probes_built() == 1); in the release library the two calls fail.
 * Registers a device buffer of `cap` 32-byte records {u32 kernel, block, HW_ID, XCC_ID; u64 t0, t1 (100 MHz)}: wave 0 of every
 * workgroup of the serial-chain kernels appends one when it ends.  d_buf == NULL switches the probe off. */
int xpnghip_debug_probe(void *d_buf, uint32_t cap);
int64_t xpnghip_debug_probe_count(void);
int xpnghip_probes_built(void);

#ifdef __cplusplus
}
#endif
#endif
