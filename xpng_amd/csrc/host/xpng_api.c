/* xpng_api.c -- host driver of the MI355X xPNG library: the drop-in for the reference's
 * xpng_store_T / xpng_load_T (libxpng.c:723-789, 963-997).
 *
 * Everything the reference driver does around its two thread fan-outs stays here, in C, with the same
 * observable behaviour: validation, normalize_RGBA, the `s <= 4 -> level 7` rule, the whole-image
 * single-colour shortcut of level 2, the RGBA level-2 -> level-1 fallback, the file header, the
 * "compressed >= raw -> rewrite as level 7" rule, and the stdout MPx/s line.  The fan-outs themselves
 * (libxpng.c:758, 983) are replaced by xpnghip_encode_tiles / xpnghip_decode_tiles (include/xpng_hip.h),
 * which run on the GPU.  There is no CPU codec in this library: if no HIP device is usable the call
 * fails (returns 1), except for the paths that never reach the tile codec (level 7, single colour).
 */
#include "../../../include/xpng.h"
#include "../../../include/xpng_hip.h"
#include "../../../include/xpng_region.h"
#include "../../../include/xpng_batch.h"
#include "../../../include/xpng_store_batch.h"
#include "../../../include/xpng_store_tensors.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define XPNG_MAX_DIM (1u << 24)

static uint64_t now_ns(void) {
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

static void put_u32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static uint32_t get_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

/* libxpng.c:688-721.  Returns 1 on allocation failure.  *out stays NULL when the raster is kept. */
static int normalize_rgba(const xpng_t *in, uint8_t **out, uint64_t *s, _Bool *A) {
    *out = NULL; *s = in->s; *A = in->A;
    if (!in->A) return 0;
    const uint64_t n = in->w * in->h;
    const uint8_t *p = in->p;
    int hidden = 0, translucent = 0;
    for (uint64_t i = 0; i < n; i++, p += 4) {
        if (p[3] == 0 && (p[0] | p[1] | p[2])) { hidden = 1; break; }
        if (p[3] != 255) translucent = 1;
    }
    if (hidden) {
        uint8_t *q = malloc(in->s);
        if (!q) return 1;
        p = in->p;
        for (uint64_t i = 0; i < n; i++, p += 4) {
            if (p[3]) memcpy(q + 4 * i, p, 4); else memset(q + 4 * i, 0, 4);
        }
        *out = q;
        return 0;
    }
    if (translucent) return 0;
    uint8_t *q = malloc(n * 3);
    if (!q) return 1;
    p = in->p;
    for (uint64_t i = 0; i < n; i++, p += 4) { q[3 * i] = p[0]; q[3 * i + 1] = p[1]; q[3 * i + 2] = p[2]; }
    *out = q; *s = n * 3; *A = 0;
    return 0;
}

static int all_pixels_equal(const uint8_t *p, uint64_t n, int pxsz) { /* whole-image form of libxpng.c:628-643; stops at the first difference */
    for (uint64_t i = 1; i < n; i++) if (memcmp(p, p + i * (uint64_t)pxsz, (size_t)pxsz)) return 0;
    return 1;
}

static _Bool write_file(const char *fn, const uint8_t hdr[8], const uint8_t *body, uint64_t len) {
    FILE *f = fopen(fn, "wb");
    if (!f) return 1;
    _Bool bad = fwrite(hdr, 1, 8, f) != 8 || (len && fwrite(body, 1, len, f) != len);
    return (_Bool)(fclose(f) != 0) || bad;
}

static void print_rate(const char *what, uint64_t workers, uint64_t ns, uint64_t pixels) {
    if (!ns) ns = 1; /* same line shape as libxpng.c:761-762 / 986-987 */
    printf("%s, %3d thread%c: %5lu MPx/s\n", what, (int)workers, workers > 1 ? 's' : ' ',
           (unsigned long)((1e9 / (double)ns) * ((double)pixels / 1e6)));
}

/* The tile-codec path of xpng_store_T (levels 1 and 2 on a raster of more than 4 bytes): the raster is uploaded once and
 * normalize_RGBA (libxpng.c:733), the whole-image single-colour test (741-753) and the tile encode (758-769) run on the
 * device.  The normalised raster comes back to the host only for the outputs that contain it verbatim. */
static _Bool store_on_device(uint64_t T, uint64_t mode, const xpng_t *pm, const char *fn, uint64_t t_start) {
    int pxsz = 0;
    xpnghip_image *img = NULL; /* this call's own staging object: concurrent xpng_store calls do not share state */
    if (xpnghip_image_begin(&img, pm->p, pm->w, pm->h, 3 + pm->A, &pxsz)) {
        fprintf(stderr, "xpng: GPU staging failed: %s\n", xpnghip_last_error());
        return 1;
    }
    const _Bool A = pxsz == 4;
    const uint64_t s = pm->w * pm->h * (uint64_t)pxsz;
    _Bool rc = 1;
    uint8_t hdr[8];
    uint8_t *raw = NULL, *blobs = NULL;
    put_u32(hdr, (uint32_t)(pm->w - 1) | ((uint32_t)mode << 24));
    put_u32(hdr + 4, (uint32_t)(pm->h - 1) | ((uint32_t)A << 24));
    if (mode == 2) { /* libxpng.c:741-753 */
        int single = 0;
        if (xpnghip_image_single_colour(img, &single)) goto done;
        if (single) {
            if (!(raw = malloc(s)) || xpnghip_image_fetch(img, raw)) goto done;
            hdr[7] |= 2;
            rc = write_file(fn, hdr, raw, (uint64_t)pxsz);
            goto done;
        }
    }
    if (A && mode == 2) { mode = 1; hdr[3] = 1; } /* libxpng.c:755 */
    if (A && (pm->w < 4 || pm->h < 4)) { /* reference behaviour undefined here: store uncompressed */
        if (!(raw = malloc(s)) || xpnghip_image_fetch(img, raw)) goto done;
        hdr[3] = XPNG_COMPRESSION_TYPE_UNCOMPRESSED;
        rc = write_file(fn, hdr, raw, s);
        goto done;
    }
    {
        uint64_t blen = 0;
        if (xpnghip_image_encode_T(img, T, (int)mode, &blobs, &blen)) {
            fprintf(stderr, "xpng: GPU tile encode failed: %s\n", xpnghip_last_error());
            goto done;
        }
        /* the reference prints its worker-thread count here (libxpng.c:761); the workers of this library are GPUs */
        print_rate("encode", (uint64_t)xpnghip_devices_for(T, pm->w, pm->h), now_ns() - t_start, pm->w * pm->h);
        if (blen >= s) { /* libxpng.c:771-777 */
            if (!(raw = malloc(s)) || xpnghip_image_fetch(img, raw)) goto done;
            hdr[3] = XPNG_COMPRESSION_TYPE_UNCOMPRESSED;
            rc = write_file(fn, hdr, raw, s);
        } else rc = write_file(fn, hdr, blobs, blen);
    }
done:
    xpnghip_image_end(img);
    free(raw);
    free(blobs);
    return rc;
}

_Bool xpng_store_T(uint64_t T, uint64_t mode, const xpng_t *pm, const char *fn) {
    const uint64_t t_start = now_ns();
    /* T: the reference's worker count (libxpng.c:146-151); here the number of GPUs of this process the tile stage may use
     * (0 = automatic), see xpnghip_encode_tiles_T */
    if (!pm || !fn || !pm->p || !pm->w || !pm->h || pm->w > XPNG_MAX_DIM || pm->h > XPNG_MAX_DIM ||
        !(mode == 1 || mode == 2 || mode == 7) || pm->w * pm->h * (3u + pm->A) != pm->s)
        return 1; /* libxpng.c:729-731 */
    /* Everything that reaches the tile codec is staged on the device.  Level 7 and rasters of at most 4 bytes after
     * normalisation (i.e. a single pixel) never do: they are handled here, on the host, and need no GPU. */
    if (mode == 2 && !pm->A && pm->w * pm->h > 1 && all_pixels_equal(pm->p, pm->w * pm->h, 3)) { /* libxpng.c:741-753, RGB input: no GPU needed */
        uint8_t h1[8];
        put_u32(h1, (uint32_t)(pm->w - 1) | (2u << 24));
        put_u32(h1 + 4, (uint32_t)(pm->h - 1));
        h1[7] |= 2;
        return write_file(fn, h1, pm->p, 3);
    }
    if (mode != 7 && pm->w * pm->h > 1) return store_on_device(T, mode, pm, fn, t_start);
    uint8_t *owned = NULL;
    uint64_t s;
    _Bool A;
    if (normalize_rgba(pm, &owned, &s, &A)) return 1;
    const uint8_t *raster = owned ? owned : pm->p;
    uint8_t hdr[8];
    mode = 7; /* explicit level 7, or s <= 4: libxpng.c:735 */
    put_u32(hdr, (uint32_t)(pm->w - 1) | ((uint32_t)mode << 24));
    put_u32(hdr + 4, (uint32_t)(pm->h - 1) | ((uint32_t)A << 24));
    const _Bool rc = write_file(fn, hdr, raster, s);
    free(owned);
    return rc;
}

_Bool xpng_store(uint64_t mode, const xpng_t *pm, const char *fn) { return xpng_store_T(0, mode, pm, fn); }

/* whole file -> malloc()ed buffer with 16 zero bytes behind it; NULL when it cannot be read or is shorter than a header */
static uint8_t *read_file(const char *fn, uint64_t *len) {
    FILE *f = fopen(fn, "rb");
    if (!f) return NULL;
    if (fseek(f, 0, SEEK_END)) { fclose(f); return NULL; }
    const long fl = ftell(f);
    if (fl < 8 || fseek(f, 0, SEEK_SET)) { fclose(f); return NULL; }
    const uint64_t flen = (uint64_t)fl;
    uint8_t *buf = malloc(flen + 16);
    if (!buf) { fclose(f); return NULL; }
    if (fread(buf, 1, flen, f) != flen) { fclose(f); free(buf); return NULL; }
    fclose(f);
    memset(buf + flen, 0, 16);
    *len = flen;
    return buf;
}

_Bool xpng_load_T(uint64_t T, const char *fn, xpng_t *pm) {
    if (!fn || !pm) return 1;
    uint64_t flen = 0;
    uint8_t *buf = read_file(fn, &flen);
    if (!buf) return 1;
    const uint64_t t_start = now_ns(); /* file read is not timed, libxpng.c:967 */
    const uint32_t h0 = get_u32(buf), h1 = get_u32(buf + 4);
    const uint64_t mode = h0 >> 24;
    pm->w = (h0 & 0xFFFFFF) + 1; pm->h = (h1 & 0xFFFFFF) + 1; pm->A = (h1 >> 24) & 1;
    if (!(mode == 1 || mode == 2 || mode == 7)) { free(buf); return 1; }
    const int pxsz = 3 + pm->A;
    pm->s = pm->w * pm->h * (uint64_t)pxsz;
    pm->p = malloc(pm->s);
    if (!pm->p) { free(buf); return 1; }
    _Bool rc = 1;
    if (mode == 7) {
        if (flen >= 8 + pm->s) { memcpy(pm->p, buf + 8, pm->s); rc = 0; }
    } else if (flen == 11u + pm->A && (buf[7] & 2)) { /* libxpng.c:976-980 */
        for (uint64_t i = 0; i < pm->w * pm->h; i++) memcpy(pm->p + i * (uint64_t)pxsz, buf + 8, (size_t)pxsz);
        rc = 0;
    } else {
        if (xpnghip_decode_tiles_T(T, (int)mode, buf + 8, flen - 8, pm->w, pm->h, pxsz, pm->p))
            fprintf(stderr, "xpng: GPU tile decode failed: %s\n", xpnghip_last_error());
        else { print_rate("decode", (uint64_t)xpnghip_devices_for(T, pm->w, pm->h), now_ns() - t_start, pm->w * pm->h); rc = 0; }
    }
    free(buf);
    if (rc) { free(pm->p); pm->p = NULL; }
    return rc;
}

_Bool xpng_load(const char *fn, xpng_t *pm) { return xpng_load_T(0, fn, pm); }

/* include/xpng_region.h: the rectangle {x, y, w, h} of the image.  The header and the two host-only forms are those of
 * xpng_load_T; levels 1 and 2 decode only the tiles the rectangle touches (xpnghip_decode_region). */
_Bool xpng_load_region(const char *fn, uint64_t x, uint64_t y, uint64_t w, uint64_t h, xpng_t *pm) {
    if (!fn || !pm) return 1;
    uint64_t flen = 0;
    uint8_t *buf = read_file(fn, &flen);
    if (!buf) return 1;
    const uint32_t h0 = get_u32(buf), h1 = get_u32(buf + 4);
    const uint64_t mode = h0 >> 24, W = (h0 & 0xFFFFFF) + 1, H = (h1 & 0xFFFFFF) + 1;
    const _Bool A = (h1 >> 24) & 1;
    const int pxsz = 3 + A;
    if (!(mode == 1 || mode == 2 || mode == 7) || !w || !h || x > W || w > W - x || y > H || h > H - y) { free(buf); return 1; }
    uint8_t *p = malloc(w * h * (uint64_t)pxsz);
    if (!p) { free(buf); return 1; }
    const uint64_t row = w * (uint64_t)pxsz;
    _Bool rc = 1;
    if (mode == 7) {
        if (flen >= 8 + W * H * (uint64_t)pxsz) {
            for (uint64_t r = 0; r < h; r++) memcpy(p + r * row, buf + 8 + ((y + r) * W + x) * (uint64_t)pxsz, row);
            rc = 0;
        }
    } else if (flen == 11u + A && (buf[7] & 2)) { /* whole-image single colour, libxpng.c:976-980 */
        for (uint64_t i = 0; i < w * h; i++) memcpy(p + i * (uint64_t)pxsz, buf + 8, (size_t)pxsz);
        rc = 0;
    } else {
        const uint64_t rect[4] = {x, y, w, h};
        if (xpnghip_decode_region((int)mode, buf + 8, flen - 8, W, H, pxsz, rect, p))
            fprintf(stderr, "xpng: GPU region decode failed: %s\n", xpnghip_last_error());
        else rc = 0;
    }
    free(buf);
    if (rc) { free(p); return 1; }
    pm->p = p; pm->w = w; pm->h = h; pm->A = A; pm->s = w * h * (uint64_t)pxsz;
    return 0;
}

/* include/xpng_batch.h: n files at once.  The header and the two host-only forms are those of xpng_load_T; the files that
 * reach the tile codec are grouped by (tile mode, bytes per pixel) and each group is decoded by mixed-size device calls
 * (xpnghip_decode_mixed).  A call takes the group's files in order until it holds 4096 images or its padded rasters - every row
 * of every image at the widest image's pitch, what the device call allocates beside ~8 B per pixel of workspace - would pass
 * XPNG_BATCH_BYTES; a file that alone passes the budget is a call of its own, as it is for xpng_load.  So a large collection costs
 * bounded device memory, and one very wide file does not widen the rows of more than one call.  No MPx/s line is printed. */
#define XPNG_BATCH_MAX 4096u
#define XPNG_BATCH_BYTES (2ull << 30)
_Bool xpng_load_batch(const char *const *paths, uint64_t n, xpng_t *out) {
    if (!paths || !out || !n) return 1;
    for (uint64_t i = 0; i < n; i++) memset(&out[i], 0, sizeof(out[i]));
    uint8_t **buf = calloc(n, sizeof(*buf));
    uint64_t *flen = calloc(n, sizeof(*flen));
    uint8_t *group = calloc(n, 1); /* 0 = answered on the host, else 1 + 2 * (mode - 1) + A */
    const uint8_t **bodies = malloc(XPNG_BATCH_MAX * sizeof(*bodies));
    uint8_t **outs = malloc(XPNG_BATCH_MAX * sizeof(*outs));
    uint64_t *lens = malloc(XPNG_BATCH_MAX * sizeof(*lens)), *dims = malloc(2 * XPNG_BATCH_MAX * sizeof(*dims));
    _Bool rc = !buf || !flen || !group || !bodies || !outs || !lens || !dims;
    for (uint64_t i = 0; !rc && i < n; i++) {
        xpng_t *pm = &out[i];
        if (!paths[i] || !(buf[i] = read_file(paths[i], &flen[i]))) { rc = 1; break; }
        const uint32_t h0 = get_u32(buf[i]), h1 = get_u32(buf[i] + 4);
        const uint64_t mode = h0 >> 24;
        pm->w = (h0 & 0xFFFFFF) + 1; pm->h = (h1 & 0xFFFFFF) + 1; pm->A = (h1 >> 24) & 1;
        if (!(mode == 1 || mode == 2 || mode == 7)) { rc = 1; break; }
        const int pxsz = 3 + pm->A;
        pm->s = pm->w * pm->h * (uint64_t)pxsz;
        if (!(pm->p = malloc(pm->s))) { rc = 1; break; }
        if (mode == 7) {
            if (flen[i] < 8 + pm->s) { rc = 1; break; }
            memcpy(pm->p, buf[i] + 8, pm->s);
        } else if (flen[i] == 11u + pm->A && (buf[i][7] & 2)) { /* libxpng.c:976-980 */
            for (uint64_t k = 0; k < pm->w * pm->h; k++) memcpy(pm->p + k * (uint64_t)pxsz, buf[i] + 8, (size_t)pxsz);
        } else group[i] = (uint8_t)(1 + 2 * (mode - 1) + pm->A);
    }
    for (uint8_t g = 1; !rc && g <= 4; g++) {
        const int mode = 1 + (g - 1) / 2, pxsz = 3 + (g - 1) % 2;
        uint64_t i = 0;
        while (!rc && i < n) {
            uint32_t k = 0;
            uint64_t rows = 0, widest = 0;
            for (; i < n && k < XPNG_BATCH_MAX; i++) {
                if (group[i] != g) continue;
                const uint64_t wd = out[i].w > widest ? out[i].w : widest;
                if (k && (rows + out[i].h) * wd * (uint64_t)pxsz > XPNG_BATCH_BYTES) break; /* the next call starts with this file */
                rows += out[i].h; widest = wd;
                bodies[k] = buf[i] + 8; lens[k] = flen[i] - 8; outs[k] = out[i].p;
                dims[2 * k] = out[i].w; dims[2 * k + 1] = out[i].h;
                k++;
            }
            if (k && xpnghip_decode_mixed(mode, pxsz, k, bodies, lens, dims, outs)) {
                fprintf(stderr, "xpng: GPU batch decode failed: %s\n", xpnghip_last_error());
                rc = 1;
            }
        }
    }
    for (uint64_t i = 0; buf && i < n; i++) free(buf[i]);
    if (rc) for (uint64_t i = 0; i < n; i++) { free(out[i].p); memset(&out[i], 0, sizeof(out[i])); }
    free(buf); free(flen); free(group); free(bodies); free(outs); free(lens); free(dims);
    return rc;
}

/* include/xpng_store_batch.h: n rasters at once.  What xpng_store_T and store_on_device decide stays here, per image and in their
 * order; the staged image becomes a staged batch (xpnghip_images_*) and the tile stage of a batch is one mixed-size device call per
 * (tile mode, bytes per pixel).  Every file's header and body are kept in memory and written only when all of them exist. */
typedef struct {
    uint8_t hdr[8];
    const uint8_t *body; /* pm->p, or `owned` */
    uint8_t *owned;
    uint64_t len;
} batch_file;

/* the second way to stage a batch: the caller's device buffers (xpng_store_tensors) instead of host rasters.  Image i of the list has
 * buffer d_bufs[i]; its size and channel count are in pms[i] (w, h, A; p is NULL) */
typedef struct {
    const void *const *d_bufs;
    uint32_t layout, dtype;
    const float *scale, *bias;
    int device;
    void *stream;
} tensor_src;

/* one staged batch: images idx[0 .. k) of the list, all of which reach the device (host rasters: levels 1 and 2, more than one
 * pixel; device buffers, ts != NULL: every image, so an explicit level 7 and the one-pixel image are here too) */
static _Bool store_batch_on_device(uint64_t mode, const xpng_t *pms, const tensor_src *ts, const uint64_t *idx, uint32_t k, batch_file *files) {
    const uint8_t **rasters = malloc(k * sizeof(*rasters));
    uint64_t *dims = malloc(2ull * k * sizeof(*dims)), *lens = calloc(k, sizeof(*lens));
    uint8_t *pin = malloc(k), *pout = malloc(k), *single = calloc(k, 1), *modes = calloc(k, 1);
    uint8_t **blobs = calloc(k, sizeof(*blobs));
    xpnghip_images *h = NULL;
    _Bool rc = 1;
    if (!rasters || !dims || !lens || !pin || !pout || !single || !modes || !blobs) goto done;
    for (uint32_t j = 0; j < k; j++) {
        const xpng_t *pm = &pms[idx[j]];
        rasters[j] = ts ? (const uint8_t *)ts->d_bufs[idx[j]] : pm->p; dims[2 * j] = pm->w; dims[2 * j + 1] = pm->h; pin[j] = (uint8_t)(3 + pm->A);
    }
    if (ts ? xpnghip_images_begin_device(&h, ts->device, k, (const void *const *)rasters, dims, pin, ts->layout, ts->dtype, ts->scale, ts->bias, ts->stream, pout)
           : xpnghip_images_begin(&h, k, rasters, dims, pin, pout)) {
        fprintf(stderr, "xpng: GPU staging failed: %s\n", xpnghip_last_error());
        goto done;
    }
    if (mode == 2 && xpnghip_images_single_colour(h, single)) goto done; /* libxpng.c:741-753 */
    for (uint32_t j = 0; j < k; j++) {
        const xpng_t *pm = &pms[idx[j]];
        batch_file *f = &files[idx[j]];
        const _Bool A = pout[j] == 4;
        const uint64_t s = pm->w * pm->h * (uint64_t)pout[j];
        put_u32(f->hdr, (uint32_t)(pm->w - 1) | ((uint32_t)mode << 24));
        put_u32(f->hdr + 4, (uint32_t)(pm->h - 1) | ((uint32_t)A << 24));
        if (mode == 7 || s <= 4) { /* explicit level 7, or s <= 4: libxpng.c:735 (host rasters never come here with either) */
            if (!(f->owned = malloc(s)) || xpnghip_images_fetch(h, j, f->owned)) goto done;
            f->hdr[3] = XPNG_COMPRESSION_TYPE_UNCOMPRESSED;
            f->body = f->owned; f->len = s;
            continue;
        }
        if (mode == 2 && single[j]) { /* the file holds one pixel: it came back with the flags, the raster stays on the device */
            if (!(f->owned = malloc(4)) || xpnghip_images_first_pixel(h, j, f->owned)) goto done;
            f->hdr[7] |= 2;
            f->body = f->owned; f->len = pout[j];
            continue;
        }
        modes[j] = (uint8_t)mode;
        if (A && mode == 2) { modes[j] = 1; f->hdr[3] = 1; } /* libxpng.c:755 */
        if (A && (pm->w < 4 || pm->h < 4)) { /* reference behaviour undefined here: store uncompressed */
            if (!(f->owned = malloc(s)) || xpnghip_images_fetch(h, j, f->owned)) goto done;
            f->hdr[3] = XPNG_COMPRESSION_TYPE_UNCOMPRESSED;
            f->body = f->owned; f->len = s;
            modes[j] = 0;
        }
    }
    if (xpnghip_images_encode(h, modes, blobs, lens)) {
        fprintf(stderr, "xpng: GPU batch encode failed: %s\n", xpnghip_last_error());
        goto done;
    }
    for (uint32_t j = 0; j < k; j++) {
        if (!modes[j]) continue;
        const xpng_t *pm = &pms[idx[j]];
        batch_file *f = &files[idx[j]];
        const uint64_t s = pm->w * pm->h * (uint64_t)pout[j];
        if (lens[j] >= s) { /* libxpng.c:771-777 */
            if (!(f->owned = malloc(s)) || xpnghip_images_fetch(h, j, f->owned)) goto done;
            f->hdr[3] = XPNG_COMPRESSION_TYPE_UNCOMPRESSED;
            f->body = f->owned; f->len = s;
        } else {
            f->owned = blobs[j]; blobs[j] = NULL;
            f->body = f->owned; f->len = lens[j];
        }
    }
    rc = 0;
done:
    xpnghip_images_end(h);
    for (uint32_t j = 0; blobs && j < k; j++) free(blobs[j]);
    free(rasters); free(dims); free(lens); free(pin); free(pout); free(single); free(modes); free(blobs);
    return rc;
}

_Bool xpng_store_batch(uint64_t mode, const xpng_t *pms, const char *const *paths, uint64_t n) {
    if (!pms || !paths || !n || !(mode == 1 || mode == 2 || mode == 7)) return 1;
    for (uint64_t i = 0; i < n; i++) { /* libxpng.c:729-731, for every image before any work */
        const xpng_t *pm = &pms[i];
        if (!paths[i] || !pm->p || !pm->w || !pm->h || pm->w > XPNG_MAX_DIM || pm->h > XPNG_MAX_DIM || pm->w * pm->h * (3u + pm->A) != pm->s) return 1;
    }
    batch_file *files = calloc(n, sizeof(*files));
    uint64_t *idx = malloc(n * sizeof(*idx));
    uint8_t *dev = calloc(n, 1); /* 1: the image reaches the tile codec */
    _Bool rc = !files || !idx || !dev;
    for (uint64_t i = 0; !rc && i < n; i++) {
        const xpng_t *pm = &pms[i];
        batch_file *f = &files[i];
        if (mode == 2 && !pm->A && pm->w * pm->h > 1 && all_pixels_equal(pm->p, pm->w * pm->h, 3)) { /* libxpng.c:741-753, RGB input */
            put_u32(f->hdr, (uint32_t)(pm->w - 1) | (2u << 24));
            put_u32(f->hdr + 4, (uint32_t)(pm->h - 1));
            f->hdr[7] |= 2;
            f->body = pm->p; f->len = 3;
            continue;
        }
        if (mode != 7 && pm->w * pm->h > 1) { dev[i] = 1; continue; }
        uint64_t s;
        _Bool A;
        if (normalize_rgba(pm, &f->owned, &s, &A)) { rc = 1; break; }
        put_u32(f->hdr, (uint32_t)(pm->w - 1) | (7u << 24)); /* explicit level 7, or s <= 4: libxpng.c:735 */
        put_u32(f->hdr + 4, (uint32_t)(pm->h - 1) | ((uint32_t)A << 24));
        f->body = f->owned ? f->owned : pm->p; f->len = s;
    }
    uint64_t nd = 0; /* the images that reach the device, in order, and where that list is cut: the chunking rule of xpng_load_batch */
    for (uint64_t i = 0; !rc && i < n; i++) if (dev[i]) idx[nd++] = i;
    if (!rc && nd > 0xFFFFFFFFull) rc = 1;
    if (!rc && nd) {
        uint64_t *dims = malloc(2 * nd * sizeof(*dims));
        uint8_t *px = malloc(nd);
        uint32_t *starts = malloc(nd * sizeof(*starts));
        int calls = -1;
        if (dims && px && starts) {
            for (uint64_t j = 0; j < nd; j++) { dims[2 * j] = pms[idx[j]].w; dims[2 * j + 1] = pms[idx[j]].h; px[j] = (uint8_t)(3 + pms[idx[j]].A); }
            calls = xpnghip_batch_cuts((uint32_t)nd, dims, px, XPNG_BATCH_MAX, XPNG_BATCH_BYTES, starts, (int)nd);
        }
        rc = calls < 1;
        for (int k = 0; !rc && k < calls; k++) {
            const uint64_t b = starts[k], e = k + 1 < calls ? starts[k + 1] : nd;
            rc = store_batch_on_device(mode, pms, NULL, idx + b, (uint32_t)(e - b), files);
        }
        free(dims); free(px); free(starts);
    }
    for (uint64_t j = 0; !rc && j < n; j++) rc = write_file(paths[j], files[j].hdr, files[j].body, files[j].len);
    for (uint64_t j = 0; files && j < n; j++) free(files[j].owned);
    free(files); free(idx); free(dev);
    return rc;
}

/* include/xpng_store_tensors.h: xpng_store_batch for images that are device buffers.  Nothing of an image is known on the host, so
 * every image is staged (xpnghip_images_begin_device quantises and rearranges it on the device) and everything xpng_store decides
 * is decided from what the staged batch reports; the list is cut as xpng_store_batch cuts it. */
_Bool xpng_store_tensors(uint64_t mode, uint64_t n, const void *const *d_bufs, const uint64_t *dims, const uint8_t *channels, uint32_t layout,
                         uint32_t dtype, const float *scale, const float *bias, int device, void *stream, const char *const *paths) {
    if (!d_bufs || !dims || !channels || !paths || !n || n > 0xFFFFFFFFull || !(mode == 1 || mode == 2 || mode == 7)) return 1;
    for (uint64_t i = 0; i < n; i++) /* (what the staged batch would refuse is refused here for the whole list, before any work) */
        if (!paths[i] || !d_bufs[i] || !dims[2 * i] || !dims[2 * i + 1] || dims[2 * i] > XPNG_MAX_DIM || dims[2 * i + 1] > XPNG_MAX_DIM ||
            (channels[i] != 3 && channels[i] != 4)) return 1;
    batch_file *files = calloc(n, sizeof(*files));
    xpng_t *pms = calloc(n, sizeof(*pms));
    uint64_t *idx = malloc(n * sizeof(*idx));
    uint32_t *starts = malloc(n * sizeof(*starts));
    const tensor_src ts = {d_bufs, layout, dtype, scale, bias, device, stream};
    _Bool rc = !files || !pms || !idx || !starts;
    int calls = -1;
    if (!rc) {
        for (uint64_t i = 0; i < n; i++) {
            idx[i] = i;
            pms[i].w = dims[2 * i]; pms[i].h = dims[2 * i + 1]; pms[i].A = channels[i] == 4; pms[i].s = pms[i].w * pms[i].h * channels[i];
        }
        calls = xpnghip_batch_cuts((uint32_t)n, dims, channels, XPNG_BATCH_MAX, XPNG_BATCH_BYTES, starts, (int)(n > 0x7FFFFFFF ? 0x7FFFFFFF : n));
        rc = calls < 1;
    }
    for (int k = 0; !rc && k < calls; k++) {
        const uint64_t b = starts[k], e = k + 1 < calls ? starts[k + 1] : n;
        rc = store_batch_on_device(mode, pms, &ts, idx + b, (uint32_t)(e - b), files);
    }
    for (uint64_t j = 0; !rc && j < n; j++) rc = write_file(paths[j], files[j].hdr, files[j].body, files[j].len);
    for (uint64_t j = 0; files && j < n; j++) free(files[j].owned);
    free(files); free(pms); free(idx); free(starts);
    return rc;
}

/* libxpng.c:1004-1014: the reference ships this entry point as a stub */
_Bool xpng_from_jpg_T(uint64_t T, const char *jpg, const char *xpng) {
    (void)T; (void)jpg; (void)xpng;
    puts("\nNot Implemented.\n");
    return 1;
}
_Bool xpng_from_jpg(const char *jpg, const char *xpng) { return xpng_from_jpg_T(0, jpg, xpng); }
