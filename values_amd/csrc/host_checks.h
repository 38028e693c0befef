// The host-side helpers every route / plan header and launcher used to carry its own copy of.  Host only, plain C++ (the route
// headers that include it compile with g++): alignment, the 128-bit type of the size guards, the two forms of the multiply-high
// magic, and the refusal macro in its two forms.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

static inline bool vx_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
static inline size_t vx_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// size and index guards: products no argument can overflow
typedef __int128 vx_wide;

// Magic of the device's multiply-high division: mulhi(i, 2^32 / d + 1) == i / d while i * d < 2^32 (the caller's guard).
//   vx_magic_or0   divisor 1 maps to 0, which vx_magic_div (common.h) reads as "no division": vx_convT_k2s2 and the 3D streaming
//                  passes, whose dimensions are often 1
//   vx_magic_raw   no such case (divisor 1 gives the word 1): vx_conv3d_k3 and vx_conv2d, whose kernels were written against this
//                  form -- their kernel arguments stay what they were
static inline unsigned vx_magic_raw(int d) { return (unsigned)((1ull << 32) / (unsigned)d) + 1u; }
static inline unsigned vx_magic_or0(int d) { return d == 1 ? 0u : vx_magic_raw(d); }

// A refusal: the message into o->err, the VX_E_* code returned; VX_REFUSE_CODE also keeps the code in o->code (the plan headers,
// whose callers read the plan after the fact)
#define VX_REFUSE(o, c, ...)                             \
  do {                                                   \
    snprintf((o)->err, sizeof((o)->err), __VA_ARGS__);   \
    return (c);                                          \
  } while (0)
#define VX_REFUSE_CODE(o, c, ...)                        \
  do {                                                   \
    snprintf((o)->err, sizeof((o)->err), __VA_ARGS__);   \
    (o)->code = (c);                                     \
    return (c);                                          \
  } while (0)
