// core.hip - what every unit of the library uses, host code only: the last error (fail, gnn_last_error), the HIP-event
// profiler behind GNN_LAUNCH (prof_pre / prof_post / ProfChain, gnn_profile_begin / gnn_profile_end), GNN_DEBUG_SYNC,
// and the entry points that describe the library itself: gnn_abi_version, gnn_shape_supported, gnn_h_stride.
#include "common.h"

namespace gnn {

thread_local char g_err[320] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

struct Profiler {
    bool on = false;
    int cap = 0;
    std::vector<hipEvent_t> ev;     // 2 per record
    std::vector<const char *> name;
    std::vector<int> start;         // index of the event a record starts at
    int n = 0;
    // Inside one library call that launches several kernels back to back (ProfChain), a kernel's
    // interval starts at the event recorded behind the previous kernel: ONE event per kernel
    // boundary, so the intervals of a call tile its time exactly - each is the kernel plus the
    // boundary to the next launch, as in an unprofiled run - instead of two event packets per
    // kernel, whose processing time (~10 us per pair) ended up inside every interval.
    bool chain = false, have_prev = false;
};
Profiler g_prof;

// GNN_DEBUG_SYNC=1: every launch is named on stderr and waited for - the last name printed before a GPU fault is
// the kernel that raised it (a debugging switch; never set in measurements)
static const char *g_dbg_name = nullptr;
static bool debug_sync()
{
    static int on = -1;
    if (on < 0) { const char *e = getenv("GNN_DEBUG_SYNC"); on = (e && e[0] == '1') ? 1 : 0; }
    return on == 1;
}

void prof_pre(const char *name, hipStream_t s)
{
    if (debug_sync()) g_dbg_name = name;
    if (g_prof.on && g_prof.n < g_prof.cap) {
        g_prof.name[g_prof.n] = name;
        if (g_prof.chain && g_prof.have_prev && g_prof.n > 0) {
            g_prof.start[g_prof.n] = 2 * (g_prof.n - 1) + 1;
        } else {
            g_prof.start[g_prof.n] = 2 * g_prof.n;
            (void)hipEventRecord(g_prof.ev[2 * g_prof.n], s);
        }
    }
}
void prof_post(hipStream_t s)
{
    if (debug_sync()) {
        fprintf(stderr, "[gnn] %s\n", g_dbg_name ? g_dbg_name : "?");
        fflush(stderr);
        (void)hipStreamSynchronize(s);
    }
    if (g_prof.on && g_prof.n < g_prof.cap) {
        (void)hipEventRecord(g_prof.ev[2 * g_prof.n + 1], s);
        g_prof.n++;
        g_prof.have_prev = true;
    }
}
ProfChain::ProfChain() : prev(g_prof.chain)
{
    if (!prev) { g_prof.chain = true; g_prof.have_prev = false; }
}
ProfChain::~ProfChain()
{
    if (!prev) g_prof.chain = g_prof.have_prev = false;
}

}  // namespace gnn

using namespace gnn;

extern "C" {

int gnn_abi_version(void) { return GNN_ABI_VERSION; }

const char *gnn_last_error(void) { return g_err; }

int gnn_shape_supported(int32_t F, int32_t D) { return ModelShapes::has(F, D); }

int32_t gnn_h_stride(int32_t F, int32_t D)
{
    return gnn_shape_supported(F, D) ? ((F + D + 3) & ~3) : 0;
}

int gnn_profile_begin(int32_t capacity)
{
    if (capacity <= 0) return fail(GNN_ERR_BADARG, "gnn_profile_begin: capacity must be positive");
    for (hipEvent_t ev : g_prof.ev) (void)hipEventDestroy(ev);
    g_prof.ev.assign(2 * (size_t)capacity, nullptr);
    g_prof.name.assign((size_t)capacity, nullptr);
    g_prof.start.assign((size_t)capacity, 0);
    g_prof.chain = g_prof.have_prev = false;
    for (auto &ev : g_prof.ev) {
        hipError_t err = hipEventCreate(&ev);
        if (err != hipSuccess) return fail(-(int)err, "hipEventCreate failed");
    }
    g_prof.cap = capacity;
    g_prof.n = 0;
    g_prof.on = true;
    return 0;
}

int gnn_profile_end(const char **names, float *ms, int32_t capacity_out)
{
    g_prof.on = false;
    const int n = g_prof.n;
    for (int i = 0; i < n; ++i) {
        hipError_t err = hipEventSynchronize(g_prof.ev[2 * i + 1]);
        if (err != hipSuccess) return fail(-(int)err, "hipEventSynchronize failed");
        if (i < capacity_out) {
            float t = 0.0f;
            (void)hipEventElapsedTime(&t, g_prof.ev[g_prof.start[i]], g_prof.ev[2 * i + 1]);
            if (ms) ms[i] = t;
            if (names) names[i] = g_prof.name[i];
        }
    }
    for (hipEvent_t ev : g_prof.ev) (void)hipEventDestroy(ev);
    g_prof.ev.clear();
    g_prof.n = 0;
    g_prof.cap = 0;
    return n;
}

}  // extern "C"
