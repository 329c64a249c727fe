// spt_jit.h — run-time specialization of the persistent kernels (spt_jit.hip). Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace spt {

// The kernels compiled per flat scene shape: every one is <kStats, kBvh = false, env, shape, tail>, kStats
// false but for the two counting k_paths of a shape with wall pairs (spt_launch_plan.h jit_kind).
enum : int { kJitPaths, kJitFrame, kJitPathsChan, kJitPathsNee, kJitFrameNee, kJitFrameRgba, kJitFrameNeeRgba,
             kJitPathsStats, kJitPathsNeeStats, kJitPathsWide, kJitPathsWideStats, kJitKinds };
constexpr int kJitCallersEnv = -1;
struct JitKindRow {
    const char* kernel;
    const char* tail;  // the template arguments after the shape
    int env;           // the kind's fixed kEnv, or kJitCallersEnv: 0 gradient sky, 1 environment map
    bool stats;        // kStats: the counting form
};
constexpr JitKindRow kJitKindTable[kJitKinds] = {
    {"k_paths", "", kJitCallersEnv},
    {"k_frame", "", kJitCallersEnv},
    {"k_paths", ", 0, true", kJitCallersEnv},        // kChan (small row shards)
    {"k_paths", ", 0, false, 1", 2},                 // kNee = kNeeAll (SPT_FLAG_NEE)
    {"k_frame", ", false, 1", 2},                    // kNee = kNeeAll
    {"k_frame", ", false, 0, true", kJitCallersEnv}, // kRgba (the fused resolve)
    {"k_frame", ", false, 1, true", 2},              // kNee = kNeeAll, kRgba
    {"k_paths", "", kJitCallersEnv, true},           // kStats
    {"k_paths", ", 0, false, 1", 2, true},           // kStats, kNee = kNeeAll
    {"k_paths", ", 0, false, 0, false, false, true", kJitCallersEnv},        // kWide (64-pixel chunks of a view)
    {"k_paths", ", 0, false, 0, false, false, true", kJitCallersEnv, true},  // kStats, kWide
};
// the name expression hiprtc instantiates for (kind, env, shape)
inline std::string jit_name_expr(int kind, int env, uint64_t shape) {
    const JitKindRow& k = kJitKindTable[kind];
    return std::string("spt::") + k.kernel + (k.stats ? "<true, false, " : "<false, false, ") +
           std::to_string(k.env == kJitCallersEnv ? env : k.env) + ", " + std::to_string((unsigned long long)shape) + "ull" + k.tail + ">";
}

// Compile the kernel for a flat scene shape (flat_shape_key) without loading it (no device needed);
// false and the compiler log on failure; `code` (optional) receives the code object. Cached per process.
bool jit_compile(int kernel, int env, uint64_t shape, std::string* log, std::vector<char>* code = nullptr);
// Which compiler the specializations use ("hiprtc MAJOR.MINOR from PATH"), or why there is none.
std::string jit_compiler();
// The loaded kernel on the current device, or nullptr. wait = true: compiled now if it is not yet
// (blocks for the compile, ~1-2 s); nullptr only if it cannot be built. wait = false: never blocks on
// the compiler — nullptr until a background compile (started by this call if none is running) has
// finished, so the caller runs its generic kernel meanwhile.
hipFunction_t jit_function(int kernel, int env, uint64_t shape, std::string* err, bool wait = true);
// Start compiling (kernel, env, shape) on a background thread unless it is compiled or compiling
// (no device needed); returns at once.
void jit_prefetch(int kernel, int env, uint64_t shape);
// true once (kernel, env, shape) has finished compiling, successfully or not.
bool jit_ready(int kernel, int env, uint64_t shape);

}  // namespace spt
