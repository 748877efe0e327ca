// seq_global_host.hpp -- what the host of mvs_seq_refine_global (capi_ba.hip) decides without the
// device: which track cuts it admits and what the device's counts mean for the limits of the sparse solver.  Plain C++ with no
// HIP in it, so that tests/cpp/seq_global_limits_check.cpp can run it on the CPU (and under the host sanitizers).
#pragma once
#include <cstdint>

#include "ba_envelope.hpp"

namespace mvs_seqg {

// max_track_frames: 0 = uncut, otherwise 2 .. 4096
inline bool track_frames_ok(int32_t T) { return T == 0 || (T >= 2 && T <= mvs_bas::kMaxFrames); }

enum Counts : int { kFits = 0, kNoPoints = 1, kTooLarge = 2 };
// the limits of mvs_ba_refine_sparse applied to the counts the device reports: points, observations, blocks of the envelope,
// pairs of observations.  A breach of any limit outranks an empty problem.
inline Counts counts_status(int64_t frames, int64_t points, int64_t obs, int64_t blocks, int64_t pairs)
{
    if (frames > mvs_bas::kMaxFrames || points > mvs_bas::kMaxPoints || obs > mvs_bas::kMaxObs ||
        blocks > mvs_pgm::kMaxEnvelopeBlocks || pairs > mvs_bas::kMaxPairs)
        return kTooLarge;
    if (points < 1 || obs < 1)
        return kNoPoints;
    return kFits;
}

}  // namespace mvs_seqg
