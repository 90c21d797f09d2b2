// learner_state.hip.h — what the two writers of the native learner-state file share: learner_state.hip (dqnhip_save_state /
// dqnhip_load_state, which defines these) and learner_save_async.hip (dqnhip_save_state_async).  The file's composition itself is
// state_codec.h's manifest; here is what it takes of a learner to fill one in.  Host only.
#pragma once
#include "learner_internal.hip.h"
#include "state_codec.h"

namespace dqnhip_host {

// v1's limits, the same for save and load
int state_refuse(const H* h, const char* what);
// what this learner's file contains when it holds `ring_size` transitions (with_mem) or none of the memory
dqnhip_state::StateShape state_shape_of(const H* h, bool with_mem, int ring_size, size_t user_bytes);
// the sections the host knows without asking the device: SOLV, LRSC, HOST, and PERC but for p_max
dqnhip_state::FixedSections state_fixed_of(const H* h);
// the ring's arrays on the device, in the order of dqnhip_state::kRingArray: pitch and width in elements of `elem` bytes
struct RingDev { void* ptr; int32_t pitch, width, elem; };
int ring_arrays_of(const H* h, RingDev out[dqnhip_state::kRingArrays]);      // -> how many this learner has (the leaves: a prioritized learner's)

}  // namespace dqnhip_host
