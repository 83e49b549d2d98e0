// launch.hpp — what the launchers of several .hip files share: the grid size
// of a one-item-per-lane launch and the dispatch on the key kind.
#pragma once
#include <stdint.h>

#include "hash.hpp"

namespace cb {

// Blocks of `per` items that cover n.
inline uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// Runs CALL with KK = the key kind as a constant (inside a function that
// returns hipError_t; an unknown kind returns hipErrorInvalidValue).
#define CB_KEY_DISPATCH(keyk, CALL)                                     \
  switch (keyk) {                                                       \
    case KEY_FIXED16: { constexpr int KK = KEY_FIXED16; CALL; } break;  \
    case KEY_FIXED: { constexpr int KK = KEY_FIXED; CALL; } break;      \
    case KEY_VAR: { constexpr int KK = KEY_VAR; CALL; } break;          \
    default: return hipErrorInvalidValue;                               \
  }

}  // namespace cb
