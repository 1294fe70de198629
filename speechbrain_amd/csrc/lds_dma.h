// The LDS-DMA piece shared by the kernels that stage tiles global -> LDS with
// global_load_lds_dwordx4 issued from inline asm: the compiler then sees no
// LDS write in flight and puts no alias-guard vmcnt wait before the LDS reads
// of the other tiles; the kernels order fills and reads with their own
// counted vmcnt waits and barriers.
#pragma once
#include "sbk_common.h"

namespace sbk {

// LDS byte address of p as a wave-uniform scalar (p must not differ by lane)
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)p));
}

// One piece: lane l's 16 bytes at src land at LDS address la + 16 l.
// (m0 is a reserved register: the clobber is advisory.  The kernels that use
// this have no other m0 user — every m0 write in their ISA is this one — so
// nothing the compiler keeps in m0 can be overwritten.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void lds_dma16(const void* src, uint32_t la) {
  asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(la) : "memory", "m0");
}
#pragma clang diagnostic pop

}  // namespace sbk
