// ct_stamps.h -- in-kernel phase stamps of the convolution kernels (s_memtime ticks per phase and wave), diagnostic builds only:
//   SRC=conv_ws tools/build_variant.sh ws_stamps -DCT_STAMPS        (one source per library; tools/prof_conv.py drives it)
// Without -DCT_STAMPS every macro below expands to nothing and the kernels are the shipping ones.
//
// A stamped wave keeps n phase totals pt[] and, at the end of the kernel, its lane 0 stores them to
//   a.prof[(block * waves + wave) * n + i]                       (CT_STAMPS_WRITE; the kernel's `lane` is the lane number)
// where a.prof is the process-wide buffer of ct_set_stamp_buffer(), copied into ConvArgs::prof by the launchers (CT_STAMPS_ARGS).
// Two forms:
//   accumulating  CT_STAMPS_BEGIN(n); CT_STAMP0(); .. CT_STAMP(i); ..
//                 CT_STAMP(i) stamps, waits for the stamp and adds the ticks since the last stamp to phase i.
//   deferred      CT_STAMPS_BEGIN_DEFERRED(n); per step: CT_STAMP_ISSUE0(); CT_STAMP_ISSUE(0) .. CT_STAMP_ISSUE(5); CT_STAMPS_AWAIT();
//                 the stamps are only ISSUED in place (a scalar memory instruction each) and awaited once, at the end of the step,
//                 so that no stamp drains the LDS queue in the middle of a phase (conv_wino4.hip: six phases per step).
#pragma once

#ifdef CT_STAMPS

namespace ct {
inline unsigned long long *g_stamp_buffer = nullptr;

template <typename Args>
inline Args with_stamp_buffer(Args a) { a.prof = g_stamp_buffer; return a; }
}  // namespace ct

// weak: a library built with the flag on more than one source still links
extern "C" __attribute__((weak)) void ct_set_stamp_buffer(unsigned long long *p) { ct::g_stamp_buffer = p; }

#define CT_STAMPS_ARGS(a) ct::with_stamp_buffer(a)
// macros, not functions: pt[] stays a set of scalar registers from the first pass of the compiler on
#define CT_STAMPS_WRITE(prof, waves, wave, n) do { if (lane == 0 && (prof)) { \
        _Pragma("unroll") for (int i__ = 0; i__ < (n); ++i__) (prof)[((size_t)blockIdx.x * (waves) + (wave)) * (n) + i__] = pt[i__]; } } while (0)

#define CT_STAMPS_BEGIN(n) unsigned long long pt[n] = {}, pt0
#define CT_STAMP0() asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pt0) :: "memory")
#define CT_STAMP(i) do { unsigned long long t__; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__) :: "memory"); pt[i] += t__ - pt0; pt0 = t__; } while (0)

#define CT_STAMPS_BEGIN_DEFERRED(n) unsigned long long pt[n] = {}, ts[10]
#define CT_STAMP_ISSUE0() asm volatile("s_memtime %0" : "=s"(ts[9]) :: "memory")
#define CT_STAMP_ISSUE(i) asm volatile("s_memtime %0" : "=s"(ts[i]) :: "memory")
#define CT_STAMPS_AWAIT() do { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(ts[0]), "+s"(ts[1]), "+s"(ts[2]), "+s"(ts[3]), "+s"(ts[4]), "+s"(ts[5]), "+s"(ts[9]) :: "memory"); \
        pt[0] += ts[0] - ts[9]; _Pragma("unroll") for (int i__ = 1; i__ < 6; ++i__) pt[i__] += ts[i__] - ts[i__ - 1]; } while (0)

#else

#define CT_STAMPS_ARGS(a) (a)
#define CT_STAMPS_WRITE(prof, waves, wave, n) do { } while (0)
#define CT_STAMPS_BEGIN(n) do { } while (0)
#define CT_STAMP0() do { } while (0)
#define CT_STAMP(i) do { } while (0)
#define CT_STAMPS_BEGIN_DEFERRED(n) do { } while (0)
#define CT_STAMP_ISSUE0() do { } while (0)
#define CT_STAMP_ISSUE(i) do { } while (0)
#define CT_STAMPS_AWAIT() do { } while (0)

#endif
