// bp_pick_token_lim_rows: bp_pick_token_lim with penalty_begin and min_length per row, for a batch whose prompts differ in length
// (src/utils/generation.py: prompt_lengths).  The kernel is pick_core.h's with its row-limited flag, in a code object of its
// own: pick_token.hip's, pick_token_ctl.hip's and pick_token_lim.hip's stay what they were.
#include "pick_core.h"

namespace bp {

hipError_t launch_pick_token_rows(const PickParams &p, int dtype, hipStream_t stream) {
    return launch_pick<RowLimited>(p, (size_t)LimLayout(p).total_words * 4, dtype, stream);   // the limited form's LDS: the arrays add nothing
}

}  // namespace bp
