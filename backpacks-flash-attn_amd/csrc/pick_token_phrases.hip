// bp_pick_token_phrases: bp_pick_token_lim_rows with banned phrases and stop phrases of several tokens, matched against the
// row's history on the device (src/utils/generation.py: bad_words_ids, stop_sequences).  The kernel is pick_core.h's with its
// phrased flag, in a code object of its own: the four other pick_token*.hip stay what they were.
#include "pick_core.h"

namespace bp {

size_t pick_phrases_lds_bytes(const PickParams &p) {
    return sizeof(PickShared) + (size_t)LimLayout(p, p.n_ban > 0).total_words * 4;
}

hipError_t launch_pick_token_phrases(const PickParams &p, int dtype, hipStream_t stream) {
    return launch_pick<Phrased>(p, (size_t)LimLayout(p, p.n_ban > 0).total_words * 4, dtype, stream);
}

}  // namespace bp
