// bbocr_page_orient: the EXIF orientation and colour order of one device page (orient.hip), as a pipeline call.
#include "ctx.h"

extern "C" {

int bbocr_page_orient(bbocr_ctx* ctx, const uint8_t* dev_src, int H, int W, long long pitch, int layout, int orientation, int dst_layout,
                      uint8_t* dev_dst, long long dst_pitch, int* out_h, int* out_w) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        check_page({dev_src, H, W, pitch, layout});
        if (!out_h || !out_w) fail(BBOCR_ERR_ARG, "null pointer");
        if (!page_orient_pair_ok(layout, dst_layout)) fail(BBOCR_ERR_ARG, "layouts: BGR or RGB from any BBOCR_PAGE_*, GRAY from GRAY");
        if (orientation < 1 || orientation > 8) fail(BBOCR_ERR_ARG, "orientation must be 1 .. 8");
        const int oh = orientation >= 5 ? W : H, ow = orientation >= 5 ? H : W;
        *out_h = oh;
        *out_w = ow;
        if (!dev_dst) return;                                    // size query
        if (dst_pitch < (long long)ow * page_px_bytes(dst_layout)) fail(BBOCR_ERR_ARG, "destination pitch smaller than a row");
        HIPCHK(launch_page_orient(dev_src, H, W, (size_t)pitch, layout, orientation, dst_layout, dev_dst, (size_t)dst_pitch, ctx->stream));
        slot_sync(ctx, ctx->stream);
    });
}

}  // extern "C"
