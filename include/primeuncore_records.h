/*
 * primeuncore_records.h — the records and constants that the host API
 * (primeuncore.h, which includes this file first) and the device engine share.
 *
 * This file, not primeuncore.h, is what the engine kernels are compiled
 * against: its text is part of every compiled configuration's identity
 * (pu_jit_source_tag).  It holds layouts only; what the entry points do with
 * these records is stated in primeuncore.h.  Plain C, no function declarations.
 */
#ifndef PRIMEUNCORE_RECORDS_H
#define PRIMEUNCORE_RECORDS_H

#include <stddef.h>
#include <stdint.h>

/* error codes */
#define PU_OK          0
#define PU_EINVAL    (-22)
#define PU_ENOMEM    (-12)
#define PU_ENODEV    (-19)
#define PU_ERANGE    (-34)
#define PU_EIO        (-5)
#define PU_ENOTSUP   (-95)
#define PU_ESTATE    (-71)   /* engine hit a state the reference treats as UB */

/* memory request types — reference src/common.h:61-66 (MemType) */
#define PU_RD 0
#define PU_WR 1
#define PU_WB 2

/* DRAM bank timing (north_star stage 4).  Opt-in, no reference counterpart:
 * the reference's Dram is a fixed latency plus a counter (dram.cpp:43-47), and
 * banks = 0 (the default; a config without a <dram> element) is exactly that.
 * With banks > 0 every Dram::access call site of System (system.cpp) becomes
 * an access to one bank of an open-page DRAM at that call's cycle t:
 *   row r = addr >> log2(row_bytes);  bank = r & (banks-1);  page = r >> log2(banks)
 *   start = max(t, bank.ready)
 *   act   = 0 (page open: row hit) | t_rcd (bank closed) | t_rp + t_rcd (other page open)
 *   delay = (start - t) + act + dram_access_time
 *   bank.ready = start + act + t_burst;  bank.open = page
 * Call sites whose Dram::access delay the reference discards (write-backs)
 * still occupy the bank.  banks and row_bytes are powers of two. */
typedef struct pu_dram_cfg {
    int32_t  banks;          /* 0 = fixed latency (the reference) */
    int32_t  t_rcd;          /* activate to column command, cycles */
    int32_t  t_rp;           /* precharge, cycles */
    int32_t  t_burst;        /* cycles a bank stays busy after the column command */
    uint64_t row_bytes;      /* bytes of one row (page) of one bank, >= 64 */
} pu_dram_cfg;

/* One request: a MsgMem record (reference src/common.h:49-59) resolved to a
 * core id and tagged with its program. */
typedef struct pu_req {
    uint64_t addr;         /* MsgMem.addr_dmem */
    int64_t  timer;        /* MsgMem.timer (core cycle when issued) */
    int32_t  core;         /* core id */
    int32_t  prog_id;      /* program (Pin process rank, >= 1) */
    uint8_t  mem_type;     /* PU_RD / PU_WR */
    uint8_t  batch_start;  /* 1 = first request of a message */
    uint16_t tag;          /* MPI tag of its message = receive-thread id (prime.cpp:53);
                              only the server's per-thread stop reads it, 0 elsewhere */
    int32_t  _pad1;
} pu_req;                  /* 32 bytes */

/* Compact 16-byte device request record: a layout of the same MsgMem fields.
 *   a = addr_dmem
 *   b = timer (bits 0-39) | core (40-55) | prog_id (56-61) | mem_type (62)
 *       | batch_start (63);  tag is 0.
 * The PU_REQ16_* constants below are that layout: PU_REQ16_B packs b from
 * fields that fit and PU_REQ16_TIMER / _CORE / _PROG / _TYPE / _BATCH take
 * them out again. */
typedef struct pu_req16 {
    uint64_t a, b;
} pu_req16;
#define PU_REQ16_TIMER_BITS 40
#define PU_REQ16_CORE_SHIFT 40
#define PU_REQ16_CORE_BITS 16
#define PU_REQ16_PROG_SHIFT 56
#define PU_REQ16_PROG_BITS 6
#define PU_REQ16_TYPE_SHIFT 62
#define PU_REQ16_BATCH_SHIFT 63
#define PU_REQ16_B(timer, core, prog_id, mem_type, batch_start)               \
    ((uint64_t)(timer) | (uint64_t)(uint32_t)(core) << PU_REQ16_CORE_SHIFT |  \
     (uint64_t)(uint32_t)(prog_id) << PU_REQ16_PROG_SHIFT |                   \
     (uint64_t)(mem_type) << PU_REQ16_TYPE_SHIFT | (uint64_t)(batch_start) << PU_REQ16_BATCH_SHIFT)
#define PU_REQ16_TIMER(b) ((int64_t)((uint64_t)(b) & (((uint64_t)1 << PU_REQ16_TIMER_BITS) - 1)))
#define PU_REQ16_CORE(b) \
    ((int32_t)(((uint64_t)(b) >> PU_REQ16_CORE_SHIFT) & (((uint64_t)1 << PU_REQ16_CORE_BITS) - 1)))
#define PU_REQ16_PROG(b) \
    ((int32_t)(((uint64_t)(b) >> PU_REQ16_PROG_SHIFT) & (((uint64_t)1 << PU_REQ16_PROG_BITS) - 1)))
#define PU_REQ16_TYPE(b) ((uint8_t)(((uint64_t)(b) >> PU_REQ16_TYPE_SHIFT) & 1u))
#define PU_REQ16_BATCH(b) ((uint8_t)((uint64_t)(b) >> PU_REQ16_BATCH_SHIFT))
#define PU_REQ_FMT_32 0    /* device request arrays hold pu_req */
#define PU_REQ_FMT_16 1    /* device request arrays hold pu_req16 */

/* bits of pu_stats.error_flags */
#define PU_ERRF_CORE_RANGE   (1ull << 0)  /* core_id >= num_cores (system.cpp:147) */
#define PU_ERRF_WB_MISS      (1ull << 1)  /* WB missed at home: NULL deref in ref (Q13) */
#define PU_ERRF_EMPTY_SHARER (1ull << 2)  /* *sharer_set.begin() on empty set */
#define PU_ERRF_QUEUE        (1ull << 3)  /* queue-model precondition violated */
#define PU_ERRF_NEG_DELAY    (1ull << 4)  /* batch delay went negative (prime.cpp:130) */
#define PU_ERRF_POOL         (1ull << 5)  /* sharer-bitmap pool exhausted (engine limit: the
                                             pool holds one entry per directory line up to
                                             2 GiB of bitmaps; PRIMEUNCORE_POOL_ENTRIES) */
#define PU_ERRF_PAGES        (1ull << 6)  /* page table 3/4 full (engine limit: 2^22 slots,
                                             raise PRIMEUNCORE_PAGE_ENTRIES) */
#define PU_ERRF_PROG         (1ull << 7)  /* no longer raised: since 0.2 directory lines
                                             carry any int prog_id (ids outside [0, 1023)
                                             escape to a side array) */
/* The engine limits and the states the reference leaves undefined: every bit
 * but CORE_RANGE and NEG_DELAY. */
#define PU_ERRF_LIMITS (PU_ERRF_WB_MISS | PU_ERRF_EMPTY_SHARER | PU_ERRF_QUEUE | \
                        PU_ERRF_POOL | PU_ERRF_PAGES | PU_ERRF_PROG)

#endif /* PRIMEUNCORE_RECORDS_H */
