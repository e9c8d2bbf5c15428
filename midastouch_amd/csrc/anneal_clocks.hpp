// anneal_clocks.hpp - phase clocks of a loop frame's kernels, in a profiling build only (tools/variants.sh ack "-DMIDAS_ANNEAL_CLOCKS";
// read out by tools/anneal_clocks.py).  Thread 0 of a kernel's first workgroup adds wall-clock ticks (100 MHz) to ctl_d[56 + i], the
// profiling block behind the control block (LoopEngine allocates 104 doubles under MIDAS_ANNEAL_CLOCKS=1).  Slot i:
//    0 ..  5  k_loop_anneal_small, from its first instruction: decision, keys, selection, compaction, duplicates sorted, written
//    6,  8    its launches that duplicated (mode 2), the sum of their k          7  its rotations workgroup
//    9        end of its extrema phase; 30 .. 34 inside that phase: own, wave, barrier, sixteen waves, equal count
//   10 .. 13  per digit pass, from the pass before: histogram zeroed, atomics, scan, pick;  14 the short finish;  15 passes
//   16 .. 20  k_loop_resample: live count known, tables built, search done, rows stored, end;  22 its launches
//   24 .. 29  k_loop_weights_moments (cluster.hip states its own)
//   35        launches of k_loop_anneal_small that reached the selection
//   36 .. 40  k_loop_xe: indices, scores, exponentials + stores, block total, end;  41 its launches
// The macros read the kernel's own names: XCK `clk` and the start `xck0`; ACK / RCK / ACKD `ctl_d` and the start `ck0` / the last
// stamp `ckl`.
#pragma once

#ifdef MIDAS_ANNEAL_CLOCKS
#define XCK(i) do { if (clk && blockIdx.x == 0 && threadIdx.x == 0) clk[56 + (i)] += (double)(wall_clock64() - xck0); } while (0)
#define XCK_COUNT(i) do { if (clk && blockIdx.x == 0 && threadIdx.x == 0) clk[56 + (i)] += 1.0; } while (0)
#define ACK(i) do { if (threadIdx.x == 0) ctl_d[56 + (i)] += (double)(wall_clock64() - ck0); } while (0)
#define ACKD(i) do { if (threadIdx.x == 0) { const long long nw = wall_clock64(); ctl_d[56 + (i)] += (double)(nw - ckl); ckl = nw; } } while (0)
#define RCK(i) do { if (blockIdx.x == 0) ACK(i); } while (0)
#define ctl_d_dbg(d, k) do { (d)[56 + 6] += 1.0; (d)[56 + 8] += (double)(k); } while (0)
#define ctl_d_pass(d) do { (d)[56 + 15] += 1.0; } while (0)
#define ctl_d_count(d, i) do { (d)[56 + (i)] += 1.0; } while (0)
#else
#define XCK(i) do { } while (0)
#define XCK_COUNT(i) do { } while (0)
#define ACK(i) do { } while (0)
#define ACKD(i) do { } while (0)
#define RCK(i) do { } while (0)
#define ctl_d_dbg(d, k) do { } while (0)
#define ctl_d_pass(d) do { } while (0)
#define ctl_d_count(d, i) do { } while (0)
#endif
