// bp_pick_token_lim: bp_pick_token_ctl with n-gram blocking, frequency / presence penalties over the row's history and a list of
// suppressed ids (the no_repeat_ngram_size / frequency_penalty / presence_penalty / suppress_tokens of the common generation
// libraries; the reference's control experiments sample with none of them).  The kernel is pick_core.h's with its limited
// flag, in a code object of its own: pick_token.hip's and pick_token_ctl.hip's stay what they were.
#include "pick_core.h"

namespace bp {

// static (PickShared) + dynamic (LimLayout: two bitmaps and the count table, each only when its control is on)
size_t pick_lim_lds_bytes(const PickParams &p) { return sizeof(PickShared) + (size_t)LimLayout(p).total_words * 4; }

hipError_t launch_pick_token_lim(const PickParams &p, int dtype, hipStream_t stream) {
    return launch_pick<Limited>(p, (size_t)LimLayout(p).total_words * 4, dtype, stream);
}

}  // namespace bp
