// The accept words of a staged round's tail and their compaction
// (abc_fused.hip), for a tail whose kernel lives in another file
// (abc_whiten.hip): candidate b is bit b % 64 of word b / 64.
#pragma once
#include "abc_common.h"

namespace abc {

struct AcceptWords { uint64_t* bits; int64_t* rtot; };
// the regions of an abc_candidates_workspace(B) buffer; false when it is too small
bool accept_words_carve(void* ws, size_t ws_bytes, int64_t B, AcceptWords& w);
// *count and the positions of the first cap accepted; the producer has
// written every word below ceil(B / 64)
int accept_words_compact(const AcceptWords& w, int64_t B, int64_t cap, int64_t* idx,
                         int64_t* count, hipStream_t s);

}  // namespace abc
