// spt_jit.h — run-time specialization of the persistent kernels (spt_jit.hip). Internal.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace spt {

// Which kernel a specialization is of, besides the flat scene's shape: k_paths or k_frame, and the code of the
// variant it instantiates (spt_launch_plan.h: paths_code / frame_code, jit_form, jit_name_expr). code < 0: none.
struct JitForm {
    bool frame;
    int code;
    explicit constexpr operator bool() const { return code >= 0; }
};
constexpr bool operator==(JitForm a, JitForm b) { return a.frame == b.frame && a.code == b.code; }

// Compile the kernel for a flat scene shape (flat_shape_key) without loading it (no device needed);
// false and the compiler log on failure; `code` (optional) receives the code object. Cached per process.
bool jit_compile(JitForm form, uint64_t shape, std::string* log, std::vector<char>* code = nullptr);
// Which compiler the specializations use ("hiprtc MAJOR.MINOR from PATH"), or why there is none.
std::string jit_compiler();
// The loaded kernel on the current device, or nullptr. wait = true: compiled now if it is not yet
// (blocks for the compile, ~1-2 s); nullptr only if it cannot be built. wait = false: never blocks on
// the compiler — nullptr until a background compile (started by this call if none is running) has
// finished, so the caller runs its generic kernel meanwhile.
hipFunction_t jit_function(JitForm form, uint64_t shape, std::string* err, bool wait = true);
// Start compiling (form, shape) on a background thread unless it is compiled or compiling
// (no device needed); returns at once.
void jit_prefetch(JitForm form, uint64_t shape);
// true once (form, shape) has finished compiling, successfully or not.
bool jit_ready(JitForm form, uint64_t shape);

}  // namespace spt
