// bp_pick_token_ctl: bp_pick_token with a repetition penalty over the row's history, an EOS mask below min_length and
// finished flags that turn a row's picks into the pad token (the reference's control baseline samples with
// repetition_penalty, training/run_pplm.py:544-550; its datasets end every document with EOS).  The kernel is pick_core.h's
// with its controlled flag, in a code object of its own: pick_token.hip's stays what it was.
#include "pick_core.h"

namespace bp {

// dynamic LDS: the history bitmap, one bit per vocabulary entry and one spare word; none without a penalty.  Above 48 KB
// (vocabularies above 393 184) launch_pick asks for the large allocation.
size_t pick_ctl_lds_bytes(const PickParams &p) { return p.theta != 1.f ? ((size_t)(p.vocab + 31) / 32 + 1) * 4 : 0; }

hipError_t launch_pick_token_ctl(const PickParams &p, int dtype, hipStream_t stream) {
    return launch_pick<Controlled>(p, pick_ctl_lds_bytes(p), dtype, stream);
}

}  // namespace bp
