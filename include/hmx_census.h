/* hmx_census.h -- launch census of libhmx.so: test instrumentation, off by default.  Part of the same C ABI as hmx.h
 * (HMX_ABI_VERSION 8: added symbols only), in its own header like hmx_device_io.h.
 *
 * The Harmony iteration is served by several hundred template instances picked at run time from the shape; the census
 * tells a test WHICH of them a run launched.  While it is enabled, every launch wrapper of the iteration kernels notes
 * the kernel function it starts in one process-wide set (all engines, all threads).  With the census off a launch costs
 * one predictable host branch; the kernels are the same either way.
 */
#ifndef HMX_CENSUS_H
#define HMX_CENSUS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: clear the set and start noting launches; on == 0: stop noting (the set stays readable).  Returns 0. */
int hmx_launch_census_enable(int on);

/* The kernels launched since the census was last enabled: their symbol names (the mangled names of the device code,
 * e.g. _Z7k_roundILi5ELi16ELb1EEv9RoundArgs), sorted, one per line, NUL-terminated, into buf[0..n).  Returns the number
 * of bytes the whole list needs including the NUL (call again with a larger buffer when that exceeds n; buf may be
 * NULL with n == 0 to ask for the size). */
int hmx_launch_census(char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* HMX_CENSUS_H */
