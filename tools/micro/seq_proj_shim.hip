// Test-only shim (tests/test_gpu_seq_proj.py): the BiLSTM input projection of a live context's 16-bit recogniser, x [rows_pad, 256] ->
// [rows_pad, 2048], through (0) crnn_seq_xproj, the helper a recognition pass calls, (1) crnn_seq_xproj_conv, the kept 1x1-conv path, and
// (2) launch_seq_proj alone, whose refusal (hipErrorNotSupported, 801) comes back as the status instead of falling through to the conv path.
// seq_proj_shim_plan reports the launcher's chunk rule for the context's device.  No kernels of its own.  Built by the test:
//   hipcc -O2 -std=c++20 -shared -fPIC --offload-arch=gfx950 -Ibb-ocr_amd/csrc -Iinclude tools/micro/seq_proj_shim.hip -Lbb-ocr_amd -lbbocr -o seq_proj_shim.so
// Pointers are device memory of caller-owned tensors with their element counts, checked before anything is launched; every call runs on
// c->stream, waits for it and returns the hipError_t as an int (0 = success), SHIM_STATUS + |code| for a StatusError of the library.
#include "ctx.h"

namespace {
constexpr int SHIM_STATUS = 10000, SHIM_UNKNOWN = 19999, SHIM_BAD_ARGS = 20000;
std::string g_err;
#define NEED(cond)                                                         \
    do {                                                                   \
        if (!(cond)) { g_err = "bad arguments: " #cond; return SHIM_BAD_ARGS; } \
    } while (0)
bool fast_rec(const bbocr_ctx* c) { return c && c->crnn_loaded && !rec_split(c) && !rec_quant(c); }
}  // namespace

extern "C" {

const char* seq_proj_shim_error() { return g_err.c_str(); }
int seq_proj_shim_rec_el(bbocr_ctx* c) { return c ? rec_el(c) : -1; }
int seq_proj_shim_xproj_channel(int dir, int gate, int unit) { return lstm8_xproj_channel(dir, gate, unit); }

// plan[5] = {workgroups, row chunks, 64-row slots in all, slots per chunk, slots of the kernel's LDS ring} of a launch over rows_pad rows on the context's device
int seq_proj_shim_plan(bbocr_ctx* c, size_t rows_pad, long long* plan) {
    g_err.clear();
    NEED(fast_rec(c) && plan && rows_pad % 256 == 0);
    if (hipError_t e = hipSetDevice(c->cfg.device); e != hipSuccess) return (int)e;
    const SeqProjPlan p = seq_proj_plan(rows_pad, device_cus());
    plan[0] = p.grid; plan[1] = p.chunks; plan[2] = p.nslots; plan[3] = p.chunk_slots; plan[4] = p.ring;
    return 0;
}

int seq_proj_shim_run(bbocr_ctx* c, int path, int layer, const uint16_t* x, size_t x_elems, size_t rows_pad, uint16_t* out, size_t out_elems) {
    g_err.clear();
    NEED(fast_rec(c) && path >= 0 && path <= 2 && (layer == 0 || layer == 1) && x && out);
    NEED(rows_pad > 0 && rows_pad % 256 == 0 && rows_pad < ((size_t)1 << 22) && x_elems == rows_pad * 256 && out_elems == rows_pad * 2048);
    try {
        hipError_t e = hipSetDevice(c->cfg.device);
        if (e != hipSuccess) return (int)e;
        c->cur = c->stream;                       // the helpers launch on c->cur; outside a guarded() call nothing has set it
        c->arena.begin(false);                    // not a dry pass; nothing is carved from the arena here
        if (path == 0) crnn_seq_xproj(c, layer, x, rows_pad, out);
        else if (path == 1) crnn_seq_xproj_conv(c, layer, x, rows_pad, out);
        else e = launch_seq_proj_profiled(c, c->xproj[layer], x, rows_pad, out);
        const hipError_t s = hipStreamSynchronize(c->stream);
        return (int)(e != hipSuccess ? e : s);
    } catch (const StatusError& se) {
        g_err = se.msg;
        (void)hipStreamSynchronize(c->stream);
        return SHIM_STATUS + std::abs(se.code);
    } catch (const std::exception& ex) {
        g_err = ex.what();
        (void)hipStreamSynchronize(c->stream);
        return SHIM_UNKNOWN;
    } catch (...) {
        g_err = "unknown failure";
        (void)hipStreamSynchronize(c->stream);
        return SHIM_UNKNOWN;
    }
}

}  // extern "C"
