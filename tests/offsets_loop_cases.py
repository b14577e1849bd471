"""What tests/test_gpu_offsets_loop.py runs, shared with tools/jit_warm.py (the
build compiles the second engine build of these configurations ahead of the
tests, so that no test waits for a compiler).

The throughput kernels form addresses into a replica's arena as the replica
base plus a 32-bit offset (engine.hip PU_OFF32, the default); -DPU_OFF32=0
keeps the 64-bit address arithmetic.  The four goldens cover the address forms
that differ: a non-power-of-two mesh, three cache levels with a bus, the 3-D
link numbering, the TLB and page-table arrays.
"""
OFFSET_GOLDENS = ("nonsquare_12", "three_level", "mesh3d", "tlb_c1")
JIT_EXTRA_OFF64 = "-DPU_OFF32=0"
LOOP_GOLDEN = "nonsquare_12"
HALT_GOLDEN = "c4_overflow_halt"
HALT_REQUESTS = 36_000      # the fixture holds 35,000: a tail past the halt to be zero-filled
