// launch.hpp — what the launchers of several .hip files share: the grid sizes
// of one-item-per-lane and grid-stride launches and the dispatches on the key
// kind and the hash mode.
#pragma once
#include <stdint.h>

#include "hash.hpp"

namespace cb {

// Blocks of `per` items that cover n.
inline uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// Grid of a grid-stride launch of kBlock-thread blocks over `items`: at least
// one block, at most cap.
constexpr uint32_t kBlock = 256;
inline uint32_t grid_for(uint64_t items, uint32_t cap = 2048) {
  uint64_t g = (items + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  return (uint32_t)(g < cap ? g : cap);
}

// Runs CALL with KK = the key kind as a constant (inside a function that
// returns hipError_t; an unknown kind returns hipErrorInvalidValue).
#define CB_KEY_DISPATCH(keyk, CALL)                                     \
  switch (keyk) {                                                       \
    case KEY_FIXED16: { constexpr int KK = KEY_FIXED16; CALL; } break;  \
    case KEY_FIXED: { constexpr int KK = KEY_FIXED; CALL; } break;      \
    case KEY_VAR: { constexpr int KK = KEY_VAR; CALL; } break;          \
    default: return hipErrorInvalidValue;                               \
  }

// Every (key kind, hash mode) instantiation, by runtime values: CALL runs
// with KK / MM as constants (inside a function that returns hipError_t).
#define CB_KEY_MODE_DISPATCH(keyk, mode, CALL)                                      \
  switch ((keyk) * 3 + (mode)) {                                                    \
    case 0: { constexpr int KK = KEY_FIXED16, MM = MOD_POW2_32; CALL; } break;      \
    case 1: { constexpr int KK = KEY_FIXED16, MM = MOD_POW2_64; CALL; } break;      \
    case 2: { constexpr int KK = KEY_FIXED16, MM = MOD_GENERIC; CALL; } break;      \
    case 3: { constexpr int KK = KEY_FIXED, MM = MOD_POW2_32; CALL; } break;        \
    case 4: { constexpr int KK = KEY_FIXED, MM = MOD_POW2_64; CALL; } break;        \
    case 5: { constexpr int KK = KEY_FIXED, MM = MOD_GENERIC; CALL; } break;        \
    case 6: { constexpr int KK = KEY_VAR, MM = MOD_POW2_32; CALL; } break;          \
    case 7: { constexpr int KK = KEY_VAR, MM = MOD_POW2_64; CALL; } break;          \
    case 8: { constexpr int KK = KEY_VAR, MM = MOD_GENERIC; CALL; } break;          \
    default: return hipErrorInvalidValue;                                           \
  }

}  // namespace cb
