/*
 * primeuncore.h — C ABI of the MI355X-native PriME uncore timing engine.
 *
 * This is the drop-in boundary for the reference's hot path
 *   UncoreManager::uncore_access  (reference src/uncore_manager.cpp:82-85)
 *     -> System::access           (reference src/system.cpp:144-168)
 * i.e. set-associative tag/LRU lookups (Cache), directory / shared-LLC MESI
 * transitions, XY mesh Network/Link timing with the Graphite history-tree +
 * M/G/1 queue model, and fixed-latency Dram (or, opt-in, a DRAM bank model
 * with no reference counterpart: pu_dram_cfg).
 *
 * Plain C: pointers, sizes and PODs only; no exceptions cross this boundary.
 * Every entry point returns 0 (or a non-negative value) on success and a
 * negative PU_E* code on failure; pu_last_error() gives the message.
 *
 * The engine keeps R independent "replicas" of the uncore on one GPU (one
 * wavefront each).  Replica r is a complete System instance; requests for
 * replica r are processed strictly in the order given (the canonical order),
 * exactly as the reference's single-threaded msgHandler loop would
 * (reference src/prime.cpp:120-137).
 */
#ifndef PRIMEUNCORE_H
#define PRIMEUNCORE_H

/* What the host shares with the device engine: the PU_E* codes, PU_RD / PU_WR /
 * PU_WB, pu_dram_cfg, pu_req, pu_req16 with PU_REQ16_* and PU_REQ_FMT_*, and
 * the PU_ERRF_* bits.  The engine kernels are compiled against that header
 * alone; this one is the host API. */
#include "primeuncore_records.h"

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PU_MAX_LEVELS 4

/* ------------------------------------------------------------------------
 * Configuration: plain-C mirror of the reference's XmlSim/XmlSys/XmlCache/
 * XmlNetwork structs (reference src/xml_parser.h:43-100), same field
 * meaning.  `cache[]` is inline (at most PU_MAX_LEVELS levels).
 * ---------------------------------------------------------------------- */
typedef struct pu_cache_cfg {          /* XmlCache, xml_parser.h:47-55 */
    int32_t  level;
    int32_t  share;
    int32_t  access_time;
    int32_t  _pad;
    uint64_t size;
    uint64_t block_size;
    uint64_t num_ways;
} pu_cache_cfg;

typedef struct pu_net_cfg {            /* XmlNetwork, xml_parser.h:57-65 */
    int32_t  data_width;
    int32_t  header_flits;
    int32_t  net_type;                 /* 0 = 2D mesh, 1 = 3D mesh */
    int32_t  _pad;
    uint64_t router_delay;
    uint64_t link_delay;
    uint64_t inject_delay;
} pu_net_cfg;

/* pu_dram_cfg, the opt-in DRAM bank model and its timing rule:
 * primeuncore_records.h. */

typedef struct pu_sys_cfg {            /* XmlSys, xml_parser.h:69-89 */
    int32_t  sys_type;                 /* 0 directory, 1 bus */
    int32_t  protocol_type;            /* 0 full map, 1 limited pointer */
    int32_t  max_num_sharers;
    int32_t  page_size;
    int32_t  tlb_enable;
    int32_t  shared_llc;
    int32_t  verbose_report;
    int32_t  dram_access_time;
    double   cpi_nonmem;
    int32_t  num_levels;
    int32_t  num_cores;
    double   freq;
    int32_t  bus_latency;
    int32_t  page_miss_delay;
    pu_net_cfg   network;
    pu_cache_cfg directory_cache;
    pu_cache_cfg tlb_cache;
    pu_cache_cfg cache[PU_MAX_LEVELS];
    pu_dram_cfg  dram;                 /* optional <dram> element; no XmlSys counterpart */
} pu_sys_cfg;

typedef struct pu_sim_cfg {            /* XmlSim, xml_parser.h:92-100 */
    int32_t  max_msg_size;
    int32_t  num_recv_threads;
    int32_t  thread_sync_interval;
    int32_t  proc_sync_interval;
    int32_t  syscall_cost;
    int32_t  _pad;
    pu_sys_cfg sys;
} pu_sim_cfg;

/* Parse a config_prime XML file (schema of reference tools/config_prime:62-198;
 * replaces XmlParser::parse, reference src/xml_parser.cpp:684-718, including its
 * required-field counts 5/13/4/6/6/6*L and the optional max_num_sharers,
 * net_type and inject_delay).  An optional <dram> element inside <system>
 * (banks, row_bytes, t_rcd, t_rp, t_burst) fills pu_sys_cfg.dram; the
 * reference's parser ignores it.  Returns 0 or PU_EINVAL. */
int pu_config_load_xml(const char* path, pu_sim_cfg* out);
int pu_config_parse_xml(const char* text, size_t len, pu_sim_cfg* out);
/* Write the config back out in config_prime's XML layout. */
int pu_config_write_xml(const pu_sim_cfg* cfg, char* buf, size_t cap, size_t* written);

/* ------------------------------------------------------------------------
 * Requests.  One pu_req per MsgMem record (reference src/common.h:49-59),
 * already resolved to a core id (ThreadSched, reference src/thread_sched.cpp:55)
 * and tagged with the Pin process rank (prime.cpp:125 prog_id = MPI source).
 * batch_start = 1 marks the first request of a MEM_REQUESTS message: the
 * running-delay rule of prime.cpp:129 restarts there:
 *     D = 0 at batch start;  d_i = access(core, req_i, timer_i + D);  D += d_i - 1
 * The record itself (32 bytes): primeuncore_records.h.
 *
 * pu_req16 (there too) is the compact 16-byte device request record for
 * throughput runs whose requests fit; no reference counterpart.  The
 * PU_REQ16_* constants are its layout, and every packer and reader of the
 * library goes through them.
 * pu_pack_req16 packs n records and returns 0, or PU_ERANGE (out untouched
 * past the record it names in the error text) at the first that does not
 * fit: timer outside [0, 2^40), core outside [0, 2^16), prog_id outside
 * [0, 64), mem_type or batch_start above 1, or tag != 0.
 * pu_set_device_req_format(h, PU_REQ_FMT_16) makes pu_run_device,
 * pu_run_device_sliced and pu_run_device_pool read d_reqs as pu_req16
 * records (indices in d_off / d_pos count records either way); those runs
 * use the throughput kernels (a latency launch's helper reads pu_req).
 * Results are identical to the same requests as pu_req.  PU_REQ_FMT_32
 * (the default) restores pu_req.  The host batch paths always take pu_req.
 * ---------------------------------------------------------------------- */

/* ------------------------------------------------------------------------
 * Statistics — every number System::report prints (reference
 * src/system.cpp:956-1111, network.cpp:310-323, dram.cpp:50-55) plus the
 * extra counters the parity harness obtains from the reference with
 * -Wl,--wrap.
 * ---------------------------------------------------------------------- */
typedef struct pu_level_stats {
    uint64_t ins;
    uint64_t miss;
    uint64_t evict;
    uint64_t wb;
} pu_level_stats;

typedef struct pu_stats {
    uint64_t net_accesses;          /* Network::num_access */
    uint64_t net_distance;          /* Network::total_distance (= link visits) */
    uint64_t net_total_delay;
    uint64_t net_router_delay;
    uint64_t net_link_delay;
    uint64_t net_inject_delay;
    uint64_t dram_accesses;
    uint64_t total_bus_contention;
    int64_t  total_num_broadcast;
    int32_t  num_levels;
    int32_t  _pad;
    pu_level_stats level[PU_MAX_LEVELS];   /* data caches, aggregated per level */
    pu_level_stats directory;              /* directory / shared-LLC slices */
    pu_level_stats tlb;
    /* extra counters */
    uint64_t link_flits;            /* sum of packet_len over Link::access */
    uint64_t mg1_calls;             /* QueueModelMG1::computeQueueDelay calls */
    uint64_t lockdown_calls;        /* Cache::lockDown calls (share/inval visits) */
    uint64_t bus_accesses;          /* Bus::access calls */
    uint64_t requests;              /* uncore_access calls */
    uint64_t error_flags;           /* PU_ERRF_* bits; 0 for a valid run */
    /* DRAM bank model (pu_dram_cfg.banks > 0; all 0 otherwise) */
    uint64_t dram_row_hits;         /* accesses to the open page of their bank */
    uint64_t dram_row_empty;        /* accesses to a closed bank */
    uint64_t dram_row_conflicts;    /* accesses that closed another page */
    uint64_t dram_bank_wait;        /* cycles spent waiting for a busy bank */
} pu_stats;

/* The PU_ERRF_* bits of error_flags: primeuncore_records.h.  PU_ERRF_LIMITS
 * are the bits that mean the replica stopped where the reference would have
 * continued (an engine limit) or reached a state the reference leaves undefined.
 * Not CORE_RANGE (System::access returns -1 and goes on) nor NEG_DELAY
 * (prime.cpp's own stop).  The host batch paths and the server return /
 * report PU_ESTATE for these. */

/* ------------------------------------------------------------------------
 * Engine lifetime and the hot path.
 * ---------------------------------------------------------------------- */
typedef struct pu_handle pu_handle;

/* Replaces UncoreManager::init (reference src/uncore_manager.cpp:46-50 ->
 * System::init system.cpp:47-141, ThreadSched::init thread_sched.cpp:44).
 * Allocates `num_replicas` independent uncores on HIP device `device`.
 * Returns NULL on failure (see pu_last_error). */
pu_handle* pu_create(const pu_sim_cfg* cfg, int num_replicas, int device);
void       pu_destroy(pu_handle* h);
/* The replica geometry the engine derives from cfg (layout offsets, set and
 * mesh parameters) as C++ source: a constexpr `Geo kJitGeo = {...};` the engine
 * can be specialised against (compile-time configuration).  Returns the full
 * length like snprintf; no reference counterpart. */
long pu_config_geo_source(const pu_sim_cfg* cfg, char* buf, size_t cap);
/* Compile-time configuration.  pu_create compiles the engine kernels for the
 * configuration's geometry with hipRTC (every cache/mesh/latency value a
 * constant) and launches that code object; compiled code objects are cached on
 * disk (PRIMEUNCORE_JIT_CACHE, else jit_cache/ beside the library).  These
 * are the library's only engine kernels: when the compile or the load fails,
 * pu_create fails and pu_last_error() carries the compiler's log.  No
 * reference counterpart (the reference's System reads its XmlSys at run time).
 * pu_config_jit_warm compiles into the cache without a GPU (1: was cached,
 * 0: compiled, PU_E* on failure).  pu_compiled_config returns 2 (the
 * compiled configuration runs every launch) for any handle and 0 for NULL;
 * other values belonged to kernels the library no longer has.
 * pu_compiled_compiler tells which compiler built the two code objects
 * (throughput and latency kernels) handle h runs: 2 hipcc for both (written
 * by pu_config_jit_warm in a process that set PRIMEUNCORE_JIT_OFFLINE=1 and
 * has not used the GPU: the build-time warm-up, tools/jit_warm.py), 1 hipRTC
 * for both (cache misses at run time), 3 one of each, 0 none. */
int pu_config_jit_warm(const pu_sim_cfg* cfg);
int pu_compiled_config(const pu_handle* h);
int pu_compiled_compiler(const pu_handle* h);
/* The symbol name of the engine kernel handle h launched last, for example
 * "pu_jit_uncore_s1_h0" (s: 0 fixed ranges, 1 time-sliced, 2 replica pool,
 * 3 resident; h: queue headers in HBM 0 or in LDS 1); a command handed to a
 * running resident kernel counts as a launch of it.  "" before any launch and
 * for NULL.  Read-only and free (the handle remembers an index): tests use it
 * to prove which kernel a call reached.  No reference counterpart. */
const char* pu_last_launch_kernel(pu_handle* h);
/* The 8-hex-digit tag of the engine sources this library compiles: the prefix
 * of every code object it writes to the cache (cache maintenance keeps the
 * code objects whose prefix some library still carries).  It covers the
 * engine's own sources only (the engine, its geometry header and
 * primeuncore_records.h), not this header: an edit here leaves the tag and
 * every cached code object as they are. */
const char* pu_jit_source_tag(void);

/* Diagnostics, no reference counterpart (tools/prof_regions.py): the
 * region cycle counters of the loaded engine kernels built
 * with PRIMEUNCORE_JIT_EXTRA=-DPU_PROF, summed over modules into out[0..n);
 * reset != 0 clears them.  Returns n, 0 when no loaded kernel counts regions,
 * < 0 on error. */
int pu_jit_prof_read(unsigned long long* out, int n, int reset);

/* Return all replicas to the just-initialised state (no reallocation). */
int        pu_reset(pu_handle* h);
int        pu_num_replicas(const pu_handle* h);
/* Device bytes held by one replica's state. */
uint64_t   pu_replica_bytes(const pu_handle* h);
/* The share of it held by the sharer-bitmap pool (full-map sets of more than
 * four LLCs).  pu_create sizes the pool exactly (one bitmap per directory line,
 * up to 2 GiB) and shrinks it, with a message on stderr, only when the
 * requested replicas would not fit the device otherwise. */
uint64_t   pu_replica_pool_bytes(const pu_handle* h);
/* Replicas this configuration's throughput kernels (time-sliced and replica
 * pool) keep resident on the device at once (one wave each; registers and LDS
 * bound it, LDS counted in the device's 1,280-B allocation units, which
 * hipOccupancy understates).  A launch over more replicas runs in several
 * rounds.  No reference counterpart (engine sizing). */
int        pu_resident_replicas(const pu_handle* h);

/* Thread -> core map (reference src/thread_sched.cpp:55-91; identical quirks:
 * first free core, a core is marked busy with prog_id, dealloc frees only
 * when core_stat == 1).  Shared by all replicas. */
int pu_alloc_core(pu_handle* h, int prog_id, int thread_id);
int pu_dealloc_core(pu_handle* h, int prog_id, int thread_id);
int pu_get_core_id(pu_handle* h, int prog_id, int thread_id);
/* The same three calls on one replica's own ThreadSched (copied from the
 * shared one on first use; the shared calls above keep updating it).  The
 * server (pu_server_*) gives every session (= replica) its own core map, as a
 * separate prime.cpp process would have.  The replica's report prints its own
 * core allocation. */
int pu_alloc_core_replica(pu_handle* h, int replica, int prog_id, int thread_id);
int pu_dealloc_core_replica(pu_handle* h, int replica, int prog_id, int thread_id);
int pu_get_core_id_replica(pu_handle* h, int replica, int prog_id, int thread_id);

/* Replay of the recorded timers (no reference counterpart; the rule is the
 * core side's, core_manager.cpp:265 `cycle += delay` after every reply):
 *   PU_REPLAY_OPEN   (default) timer_i is used as recorded;
 *   PU_REPLAY_CLOSED timer_i += the sum of the batch delays of that core's
 *                    earlier messages, as if the recording core had waited for
 *                    each reply.  The uncore (System) is untouched. */
#define PU_REPLAY_OPEN   0
#define PU_REPLAY_CLOSED 1
int pu_set_replay_mode(pu_handle* h, int mode);

/* PU_ERRF_* bits of replicas [0, n) (EngineStats.error_flags). */
int pu_error_flags(pu_handle* h, uint64_t* out, size_t n);
/* For replicas [0, n): the index, into the last launch's request array, of
 * the first request that raised a PU_ERRF_LIMITS bit (UINT64_MAX: none).
 * Every request before it was simulated exactly (the server still answers
 * the messages that ended before it). */
int pu_limit_positions(pu_handle* h, uint64_t* out, size_t n);

/* Single-request compatibility path: UncoreManager::uncore_access
 * (uncore_manager.cpp:82-85).  Operates on replica 0; `*addr` is updated in
 * place like InsMem::addr_dmem (system.cpp:916).  Returns the delay (an int,
 * negative when the reference's int wraps) or -1 for core_id >= num_cores,
 * like System::access (system.cpp:147-150).  No prime.cpp halt rule and no
 * closed-loop shift apply here: those belong to the caller's message loop. */
int pu_access(pu_handle* h, int core_id, int prog_id, int mem_type,
              uint64_t* addr, int64_t timer);
/* The same with the status out of band: returns 0 or PU_E*, and the delay
 * (any int, including a wrapped negative one, or -1 for core_id >= num_cores)
 * goes to *delay_out.  pu_access reports errors in-band, so a wrapped delay
 * that happens to equal a PU_E* code is ambiguous there; the C++ and Python
 * mirrors use this entry point. */
int pu_access_status(pu_handle* h, int core_id, int prog_id, int mem_type,
                     uint64_t* addr, int64_t timer, int32_t* delay_out);

/* Batch path from host memory: the per-message loop of prime.cpp:120-137 for
 * replica `replica`.  delay_out[i] receives uncore_access's return value for
 * reqs[i] (may be NULL).  Synchronous.  Returns 0 or PU_E*; PU_ESTATE when
 * the replica carries a PU_ERRF_LIMITS bit (an engine limit stopped it where
 * the reference would continue: later delays are 0, not the reference's). */
int pu_access_batch(pu_handle* h, int replica, const pu_req* reqs, size_t n,
                    int32_t* delay_out);

/* Resident mode (no reference counterpart; the transport under prime.cpp:129's
 * per-request uncore_access and the per-message batch): pu_access,
 * pu_access_status and pu_access_batch of at most 16,384 requests do not
 * launch a kernel per call.  The first such call starts one persistent
 * latency-mode workgroup for that replica, which keeps the replica's queue
 * headers in its CU's LDS and takes every later call through a mailbox in
 * host-coherent pinned memory (requests in, delays and error flags out), each
 * call computing exactly what one launch would.  It leaves by itself after
 * PRIMEUNCORE_RESIDENT_IDLE_MS (default 50) without a call, when another
 * replica or a launch of any kind needs the engine, on pu_reset, pu_synchronize,
 * a read of statistics, completion cycles or the report, and on pu_destroy or
 * process exit.  It needs the compiled configuration and a replica whose queue
 * headers fit one CU's LDS; otherwise (or with PRIMEUNCORE_RESIDENT=0) every
 * call launches as before.  pu_set_resident: mode 1 on, 0 off (joins a running
 * kernel), -1 query; returns the previous mode.  pu_resident_info writes up
 * to n of {kernel running, commands served, kernels launched, eligible, then
 * summed over the commands: the kernel's request-copy, message-loop, close
 * (run state and counters) and mailbox phases in 10-ns ticks (commands with a
 * full answer), the host's post-to-answer time in ns, and how many commands
 * came back as the fast answer (one request, no new error bit, no TLB: the
 * delay and the command number in one 8-B store)} and returns how many it
 * wrote. */
int pu_set_resident(pu_handle* h, int mode);
int pu_resident_info(pu_handle* h, uint64_t* out, size_t n);

/* Batch path from device memory, all replicas at once, asynchronous on
 * `hip_stream` (a hipStream_t; NULL = the engine's own stream, see
 * pu_synchronize).  Replica r
 * processes d_reqs[d_off[r] .. d_off[r+1]) and writes d_delay over the same
 * range.  d_off holds num_replicas+1 entries and lives in device memory.
 * Nothing is copied to or from the host. */
int pu_run_device(pu_handle* h, const pu_req* d_reqs, const uint64_t* d_off,
                  int32_t* d_delay, void* hip_stream);
/* Time-sliced variant for throughput runs of many replicas: replica r
 * processes d_reqs[d_pos[r] .. d_off[r+1]) in order but stops before the first
 * request that would start more than budget_us microseconds (wall clock) after
 * its wavefront started, and writes its next position back to d_pos[r]
 * (device memory, num_replicas entries).  A replica stops only between
 * requests, so calling again continues its stream exactly; results are the
 * same as one unsliced run over the same requests.  budget_us = 0: no limit. */
int pu_run_device_sliced(pu_handle* h, const pu_req* d_reqs, const uint64_t* d_off,
                         int32_t* d_delay, uint64_t* d_pos, uint64_t budget_us, void* hip_stream);
/* Replica pool: pu_run_device_sliced for more replicas than run at once (no
 * reference counterpart; throughput runs).  A launch runs `slots` wavefronts,
 * 1 <= slots <= pu_pool_slots(h) = min(num_replicas, pu_resident_replicas).
 * Each slot continues the replica it held when the previous pool launch
 * ended; a slot whose replica is done (d_pos[r] reached d_off[r+1], or the
 * replica stopped by the prime.cpp:130-134 rule: the rest of its range reads
 * 0) takes the next replica nobody has started, in index order, and goes on
 * within the same slice, so no wavefront idles while unstarted replicas
 * remain.  Per replica the results are those of pu_run_device_sliced (each
 * replica is processed in order, by one wavefront at a time).  d_sched:
 * pu_pool_words(slots) = B + 2*slots uint32 words of device memory,
 * B = (3 + slots) & ~1, all 0 before the first launch of a pool run, the same
 * slots for every launch of it (word 0 = replicas taken so far; word 1
 * unused; then per slot its replica + 1; from word B, per slot one uint64:
 * the 100-MHz ticks its wavefronts have been resident, summed over launches:
 * the busy time of the pool).
 * budget_us > 0. */
int  pu_pool_slots(pu_handle* h);
long pu_pool_words(int slots);
int  pu_run_device_pool(pu_handle* h, const pu_req* d_reqs, const uint64_t* d_off, int32_t* d_delay,
                        uint64_t* d_pos, uint32_t* d_sched, int slots, uint64_t budget_us, void* hip_stream);
int pu_set_device_req_format(pu_handle* h, int fmt);
int pu_pack_req16(const pu_req* in, size_t n, pu_req16* out);
int pu_synchronize(pu_handle* h);

/* Per-core completion cycle of the last request each core issued
 * (last timer_i + D + d_i); out has num_cores entries (-1 = no request). */
int pu_core_completion(pu_handle* h, int replica, int64_t* out, size_t n);

/* Statistics and the report text of UncoreManager::report
 * (uncore_manager.cpp:87-98 -> ThreadSched::report, System::report) for one
 * replica.  With include_time == 0 the wall-clock line is omitted so the
 * text can be compared byte-for-byte.  Returns the full length (like
 * snprintf); writes at most cap bytes including the terminating NUL. */
int pu_stats_get(pu_handle* h, int replica, pu_stats* out);
long pu_report(pu_handle* h, int replica, int include_time, char* buf, size_t cap);

/* Device-time of the last pu_run_device / pu_access_batch launch, in ms,
 * measured with HIP events on the engine's stream (a call served by the
 * resident kernel: its wall time from posting to the answer). */
double pu_last_kernel_ms(pu_handle* h);

/* UncoreManager::getSimStartTime / getSimFinishTime (uncore_manager.cpp:52-60):
 * wall-clock stamps (CLOCK_REALTIME); pu_report(include_time=1) prints their
 * difference as "Total computation time" like UncoreManager::report (:92-93). */
void pu_sim_start_time(pu_handle* h);
void pu_sim_finish_time(pu_handle* h);

const char* pu_last_error(void);
const char* pu_version(void);

/* ------------------------------------------------------------------------
 * Synthetic request streams.  Deterministic: one splitmix64
 * per core seeded seed*2^32 + core; per core timer += 1 + U{0..3}; a core
 * stops at each quantum barrier (q+1)*quantum (core_manager.cpp:104-198);
 * messages of <= max_msg requests never span a barrier; canonical order is
 * quantum-major, then core id, batch-atomic.
 * ---------------------------------------------------------------------- */
#define PU_STREAM_PRIVATE_STREAMING 1  /* C1: blackscholes-like */
#define PU_STREAM_SHARED_UNIFORM    2  /* C2: canneal-like */
#define PU_STREAM_MULTIPROGRAM      3  /* C3: SPEC-like mix, 4 programs */
#define PU_STREAM_UNIFORM_HOTSPOT   4  /* C4: uniform 2^20 lines + 64-line hotspot */
#define PU_STREAM_PRODUCER_CONSUMER 5  /* C5: core pairs sharing buffers */
#define PU_STREAM_UNIFORM           6  /* C4(i): pure uniform */

typedef struct pu_stream_params {
    int32_t  kind;             /* PU_STREAM_* */
    int32_t  num_cores;
    uint64_t seed;
    int32_t  quantum;          /* thread_sync_interval, e.g. 1000 */
    int32_t  num_quanta;       /* quanta to generate */
    int32_t  max_msg;          /* max_msg_size, e.g. 100 */
    int32_t  num_progs;        /* programs; core c belongs to prog 1 + c*num_progs/num_cores */
    int64_t  max_requests;     /* stop after this many requests (<=0: no cap) */
    int32_t  write_pct;        /* percent writes; <0 = kind default */
    int32_t  _pad;
} pu_stream_params;

/* Number of requests the stream holds (call first to size the buffer). */
int64_t pu_stream_count(const pu_stream_params* p);
/* Fill out[0..cap) in canonical order; returns the number written or PU_E*. */
int64_t pu_stream_generate(const pu_stream_params* p, pu_req* out, size_t cap);
/* The (prog_id, thread_id) of core c in a generated stream. */
int pu_stream_thread_of(const pu_stream_params* p, int core, int* prog_id, int* thread_id);

/* Resumable streams: the same requests as pu_stream_generate, produced in
 * consecutive chunks (concatenating the chunks gives exactly the one-shot
 * stream).  pu_stream_next returns the number written (< n at the end).
 * pu_stream_next_many advances `count` streams by up to n_each requests each
 * on `threads` host threads (<= 0: all cores), stream i writing
 * out[i*stride ...]; returns the smallest count written. */
typedef struct pu_stream pu_stream;
pu_stream* pu_stream_open(const pu_stream_params* p);
void       pu_stream_close(pu_stream* s);
int64_t    pu_stream_next(pu_stream* s, pu_req* out, size_t n);
int64_t    pu_stream_position(const pu_stream* s);
int64_t    pu_stream_next_many(pu_stream* const* s, int count, pu_req* out, size_t n_each,
                               size_t stride, int threads);

/* 0 when every record of the stream fits pu_req16, else PU_ERANGE (PU_EINVAL for
 * parameters pu_stream_open refuses); no reference counterpart.  Decided from the
 * parameters alone (a timer is below num_quanta*quantum, a core below num_cores, a
 * program at most max(num_progs, 1)): it may refuse a stream that would happen to
 * fit, and never accepts one that pu_pack_req16 would refuse. */
int pu_stream_fits_req16(const pu_stream_params* p);

/* Streams generated on the device (no reference counterpart; the first stage of a
 * device-side ensemble: pu_dstream_next -> pu_run_device / _sliced / _pool with no
 * request ever on the host).
 *
 * pu_dstream_open: `count` streams (params[i] may differ in every field, num_cores
 * included) whose generator state lives in device memory of `device`: per stream a
 * small header, 24 B per core, and for PU_STREAM_SHARED_UNIFORM streams 132 B per
 * core more (the re-use ring).  Validates every params[i] (the rule of
 * pu_stream_open) before touching a device; NULL + pu_last_error() on failure ("no
 * HIP device" where there is none, as pu_create; PU_ENOMEM with the size asked for
 * when the device memory cannot be had).
 *
 * pu_dstream_next: the next up to n_each requests of every stream: stream i writes
 * records d_out[i*stride .. i*stride + got_i) (indices in records of the chosen
 * format), where got_i = min(n_each, what the stream has left) and the records are
 * exactly those that pu_stream_next would return for the same stream at the same
 * position -- as pu_req (fmt = PU_REQ_FMT_32: all 32 bytes written, tag and padding
 * 0) or as pu_pack_req16 of them (PU_REQ_FMT_16).  Records past got_i, and the gap
 * between n_each and stride, are not written.  d_got (device, count uint64, may be
 * NULL) receives got_i.  Asynchronous on hip_stream (NULL = the set's own stream);
 * calls on one set are ordered on the host (the caller does not issue two at once),
 * and a call on another stream than the one before runs after it on the device.
 * stride >= n_each; d_out 16-byte aligned.  Returns 0 or PU_E*; PU_ERANGE with a
 * message, before anything is launched, for PU_REQ_FMT_16 when a stream of the set
 * does not pass pu_stream_fits_req16 (PU_REQ_FMT_32 still serves that set).
 *
 * pu_dstream_positions: requests produced so far per stream (pu_stream_position)
 * for streams [0, n); waits for the set's outstanding calls first.
 * pu_dstream_state_bytes: device memory the set holds.
 *
 * pu_dstream_positions and pu_dstream_close wait only for the work of this set (the
 * event of its last call), never for the device (no hipDeviceSynchronize): next to
 * another handle's resident kernel a device-wide wait lasts until that kernel idles
 * out.  pu_dstream_close then frees the set's memory, and hipFree may itself wait
 * for the whole device. */
typedef struct pu_dstream pu_dstream;
pu_dstream* pu_dstream_open(const pu_stream_params* params, int count, int device);
void        pu_dstream_close(pu_dstream* s);
int         pu_dstream_next(pu_dstream* s, void* d_out, size_t n_each, size_t stride, int fmt,
                            uint64_t* d_got, void* hip_stream);
int         pu_dstream_positions(pu_dstream* s, int64_t* out, size_t n);
uint64_t    pu_dstream_state_bytes(const pu_dstream* s);

/* Delay summaries kept on the device (no reference counterpart; the last stage of a
 * device-side ensemble: pu_dstream_next -> pu_run_device / _sliced / _pool ->
 * pu_dsum_add, with no request and no delay ever on the host).  Every figure is an
 * exact integer and independent of the order of the records, so the device result
 * equals the host fold (pu_dsum_host_add) bit for bit.
 *
 * The rule (primesim_amd/csrc/delay_sum_step.h):
 *   class    0 = read, 1 = write.  pu_req16: bit 62 of b.  pu_req: 1 where mem_type ==
 *            PU_WR, else 0 -- the engine hands mem_type on unchanged and takes its
 *            write path only for PU_WR, so PU_RD, PU_WB and any other value are class 0.
 *   bucket   of a delay d (int32): 0 for d <= 0, else 32 - clz(d): 1 -> 1, 2..3 -> 2,
 *            4..7 -> 3, ..., 2^30..2^31-1 -> 31.  Bucket 0 holds the zeros that a stopped
 *            replica's remaining range reads, the -1 of a core id out of range, and
 *            delays that wrapped negative.
 *   class    count, sum (exact, over every delay, non-positive ones included), min and
 *            max (an empty class: INT32_MAX / INT32_MIN), hist[bucket].
 *   replica  the two classes and core_out_of_range: the records whose core id is < 0 or
 *            >= the replica's num_cores (without num_cores: < 0 only).  Such a record
 *            still counts in its class and touches no per-core entry.
 *   core     (optional) count and sum of the delays of the core's requests, both
 *            classes together.
 *
 * pu_dsum_open: `count` replicas; num_cores NULL: no per-core tables, else `count`
 * entries, each >= 1.  State in device memory of `device`: 568 B per replica; with
 * tables 12 B per replica and 16 B per core more.  Arguments are validated before a device is
 * touched; NULL + pu_last_error() on failure ("no HIP device" where there is none, PU_ENOMEM
 * with the size asked for).
 *
 * pu_dsum_add: replica r folds records [d_begin[r], d_end[r]) of d_reqs (pu_req, or
 * pu_req16 with fmt = PU_REQ_FMT_16; 16-byte aligned) and d_delay into its running
 * summary; indices count records as in d_off / d_pos, both index arrays are in device
 * memory with `count` entries, and d_begin[r] >= d_end[r] adds nothing.  d_off and
 * d_off + 1 summarise a pu_run_device launch; a copy of d_pos saved before a sliced or
 * pool launch and d_pos after it summarise exactly what that launch simulated.
 * Asynchronous on hip_stream (NULL = the set's own stream); calls on one set are ordered
 * on the host by the caller, and a call on another stream than the one before runs after
 * it on the device.  Returns 0 or PU_E*.
 *
 * pu_dsum_read: summaries of replicas [first, first + n).  pu_dsum_read_cores: the first
 * n (<= num_cores) per-core counts and sums of one replica (either output may be NULL);
 * PU_EINVAL for a set opened without tables.  pu_dsum_reset: back to the state after open.
 * pu_dsum_state_bytes: device memory the set holds.  pu_dsum_read, _read_cores, _reset and
 * _close wait only for the work of this set (the event of its last call), never for the
 * device, for the reason given for pu_dstream_* above.  A NULL set: PU_EINVAL, 0, no-op.
 *
 * pu_dsum_host_init / pu_dsum_host_add: the same fold over host arrays, for users of
 * pu_access_batch; needs no device.  core_count / core_sum: both NULL, or num_cores (>= 1)
 * entries each; num_cores <= 0 (tables NULL): only negative core ids are out of range. */
#define PU_DSUM_BUCKETS 32
typedef struct pu_dsum_class {
    uint64_t count;
    int64_t  sum;
    int32_t  min, max;
    uint64_t hist[PU_DSUM_BUCKETS];
} pu_dsum_class;               /* 280 bytes */
typedef struct pu_dsum_replica {
    pu_dsum_class cls[2];
    uint64_t core_out_of_range;
} pu_dsum_replica;             /* 568 bytes */

typedef struct pu_dsum pu_dsum;
pu_dsum* pu_dsum_open(int count, const int32_t* num_cores, int device);
void     pu_dsum_close(pu_dsum* s);
int      pu_dsum_add(pu_dsum* s, const void* d_reqs, int fmt, const int32_t* d_delay,
                     const uint64_t* d_begin, const uint64_t* d_end, void* hip_stream);
int      pu_dsum_read(pu_dsum* s, int first, int n, pu_dsum_replica* out);
int      pu_dsum_read_cores(pu_dsum* s, int replica, uint64_t* count_out, int64_t* sum_out, size_t n);
int      pu_dsum_reset(pu_dsum* s);
uint64_t pu_dsum_state_bytes(const pu_dsum* s);
void     pu_dsum_host_init(pu_dsum_replica* acc);
int      pu_dsum_host_add(pu_dsum_replica* acc, uint64_t* core_count, int64_t* core_sum, int num_cores,
                          const void* reqs, int fmt, const int32_t* delays, size_t n);

/* End-of-run results gathered on the device (no reference counterpart; the fourth stage of
 * a device-side ensemble: pu_dstream_next -> pu_run_device / _sliced / _pool ->
 * pu_dsum_add -> pu_dres_gather).  One kernel launch reads, for every replica of a range,
 * what pu_stats_get and pu_core_completion would copy one replica at a time, plus the
 * engine's exact visit counts per link and bus, into one dense record per replica; one
 * copy brings the records to the host.  A gather is a snapshot, not an accumulator:
 * gathering twice without a run in between gives the same bytes.  Every figure is an
 * integer, so the device record equals pu_dres_host_gather's byte for byte.
 *
 * The rules (primesim_amd/csrc/run_results_step.h):
 *   queues      [0, nlinks) are the links, [nlinks, nqueues) the buses, in the engine's
 *               record numbering (pu_config_queue_ends).  For a link, n counts all visits
 *               and n1 the visits of block-length packets: the flits sent over it are
 *               header_flits * n + (plen_blk - header_flits) * n1, where plen_blk =
 *               header_flits + ceil(last-level block size / data_width).  A bus carries one
 *               packet length (bus_latency), so its n1 is reported as 0.
 *   busiest     link_max_* / bus_max_*: the largest n of the range and, among equal
 *               counts, the lowest queue id (a bus's id counts from nlinks as in the map).
 *               A configuration without links (buses) reports id -1 and 0 visits; one with
 *               links none of which was visited reports 0 visits at id 0 (nlinks for buses).
 *               links_used / buses_used count the queues with n > 0.
 *   completion  over the cores that have completed a request, i.e. whose cycle is not the
 *               -1 that a reset writes and pu_core_completion returns for an idle core:
 *               cores_done of them, completion_max (the simulated end cycle), _min and
 *               _sum; with none: INT64_MIN, INT64_MAX and 0.
 *   stats       field for field what pu_stats_get returns.
 *
 * pu_dres_open: a set for all replicas of h, on h's device.  flags: 0, or PU_DRES_QUEUES
 * to keep the per-queue map (n and n1 of every queue of every replica: 16 B per queue and
 * replica on top of the 448-B records, e.g. 31,744 B per replica of a 32x32 mesh, which is
 * why it is optional).  The set must be closed before h is destroyed.
 *
 * pu_dres_gather: replicas [first, first + n), asynchronous on hip_stream (NULL = the
 * set's own stream).  Ordering: the caller orders a gather after the run it wants to see --
 * the same stream, or pu_synchronize first; a gather orders itself after the set's earlier
 * calls whatever stream they were on.  It first joins a resident kernel of h (whose queue
 * headers live on chip until it leaves).  The other replicas' records and map rows stay as
 * they were.
 *
 * pu_dres_read: records of replicas [first, first + n).  pu_dres_read_queues: n and n1 of
 * every queue of one replica as of its last gather (either output may be NULL; cap >=
 * nqueues entries each); PU_ENOTSUP for a set opened without PU_DRES_QUEUES.
 * pu_dres_read_queue_totals: per queue, the sums of n and n1 over the replicas of the last
 * gather that was launched (all zero before the first, and after a gather of no replica),
 * by two more launches without atomics on the set's own stream, after that gather.  A set
 * with the map sums the map: a snapshot, like the records.  A set without it sums the queue
 * headers as they are at this call: after another run the two kinds of set answer
 * differently for the same gather, so read the totals before the next run, or keep the
 * map.  pu_dres_read*, and pu_dres_close, wait only for the work
 * of this set (the event of its last call), never for the device.
 *
 * pu_dres_host_gather: the same record, and optionally the same n / n1 rows, for one
 * replica by plain copies (pu_stats_get, pu_core_completion, and copies of the run state and
 * the queue headers).  pu_num_links / pu_num_queues: links / queues (links, then buses) per
 * replica of a handle; pu_dres_nqueues: the queues of a set's replicas (0 for NULL).  pu_dres_state_bytes: device memory the set holds.
 *
 * pu_config_queue_ends: which edge or bus queue q of cfg is; host only, needs no device.
 * kind 0 / 1 / 2: a link along x / y / z between the network nodes a < b; 3: a bus, a =
 * its cache level, b = the cache's index in that level; -1 (a = b = -1): q names no queue.
 * Node (x, y, z) of a mesh of width w has id z*w*w + y*w + x.  2-D: record y*(w-1) + x_low
 * is the x link between (x_low, y) and (x_low + 1, y); record w*(w-1) + x*(w-1) + y_low
 * the y link between (x, y_low) and (x, y_low + 1).  3-D: three blocks of w*w*(w-1)
 * records: x at (z*w + y)*(w-1) + x_low, y at (z*w + x)*(w-1) + y_low, z at
 * (y*w + x)*(w-1) + z_low.  The records cover the whole w x w (x w) grid even where the
 * configuration has fewer nodes.
 *
 * Arguments are checked before any device call: a NULL handle or set, unknown flags:
 * PU_EINVAL; first < 0, n < 0: PU_EINVAL; first + n > replicas, a replica out of range,
 * cap too small: PU_ERANGE.  Returns 0 or PU_E*. */
#define PU_DRES_QUEUES 1            /* keep the per-queue map [R][nqueues] */
typedef struct pu_dres_replica {
    pu_stats stats;                 /* field for field what pu_stats_get returns */
    uint64_t processed;             /* RunState.processed */
    int32_t  halted, cores_done;    /* RunState.halted; cores that have completed a request */
    int64_t  completion_max, completion_min, completion_sum;
    uint64_t link_visits, link_block_visits;   /* sum of n and of n1 over the links */
    uint64_t link_max_visits;
    int32_t  link_max_id, links_used;
    uint64_t bus_visits, bus_max_visits;
    int32_t  bus_max_id, buses_used;
} pu_dres_replica;                  /* 448 bytes */

typedef struct pu_dres pu_dres;
pu_dres* pu_dres_open(pu_handle* h, int flags);
void     pu_dres_close(pu_dres* s);
int      pu_dres_gather(pu_dres* s, int first, int n, void* hip_stream);
int      pu_dres_read(pu_dres* s, int first, int n, pu_dres_replica* out);
int      pu_dres_read_queues(pu_dres* s, int replica, uint64_t* n_out, uint64_t* n1_out, size_t cap);
int      pu_dres_read_queue_totals(pu_dres* s, uint64_t* n_out, uint64_t* n1_out, size_t cap);
int      pu_dres_nqueues(const pu_dres* s);
uint64_t pu_dres_state_bytes(const pu_dres* s);
int      pu_num_links(const pu_handle* h);
int      pu_num_queues(const pu_handle* h);
int      pu_dres_host_gather(pu_handle* h, int replica, pu_dres_replica* out,
                             uint64_t* n_out, uint64_t* n1_out, size_t cap);
int      pu_config_queue_ends(const pu_sim_cfg* cfg, int q, int* kind, int* a, int* b);

/* Forking a warmed replica and its request stream (no reference counterpart; for ensembles
 * that would otherwise simulate the same cold start once per replica: warm one replica,
 * then branch it).
 *
 * pu_replica_fork: replicas [first, first + n) of h become bit-for-bit copies of replica
 * src, as the arena holds it when the call's work runs on hip_stream (NULL = the engine's
 * own stream, as for pu_run_device).  Asynchronous: the caller orders it against its runs
 * by the stream, as for pu_run_device.  src inside the range is skipped and left as it is
 * (so src = 0, first = 0, n = num_replicas is legal); n == 0 is a successful no-op.  The
 * copy is the whole replica: cache and directory lines, the sharer pool and its free
 * stack, queue headers and rings, TLBs and the page map, the counters with the error
 * flags, completion cycles, the run state (an open message's running delay, halted, the
 * limit position), the closed-loop core shifts and the DRAM banks.  A destination's
 * pu_stats_get, pu_report, pu_core_completion, pu_error_flags, pu_limit_positions and
 * pu_dres_* records therefore equal the source's right after the fork: they include the
 * warm-up's counts, and a caller who wants the figures of the measured part alone
 * subtracts the source's figures as of the fork.  A running resident kernel is joined first
 * (the source's queue headers are then in device memory).  If src has its own thread
 * scheduler (pu_*_core_replica) every destination gets a copy of it; otherwise a
 * destination's own copy is dropped and it reads the shared one, as src does.  d_pos and
 * d_sched of the sliced and pool launches are the caller's: a forked destination starts
 * wherever the caller's d_pos says.  By default one kernel reads the source in 16-KiB
 * tiles and stores each tile to every destination; PU_FORK_BY_COPIES does the same by one
 * device-to-device copy per destination on the same stream.  Forks share their warm-up:
 * they are correlated until their own streams have displaced it.
 * Before anything is launched: PU_EINVAL for a NULL handle, a negative argument or
 * unknown flags; PU_ERANGE for src or the range outside [0, num_replicas).
 *
 * pu_stream_fork / pu_dstream_fork: the stream that goes with a forked replica.  A fresh
 * stream starts at cycle 0, in the past of a warmed replica, so the destination takes
 * from the source its cursor (quantum, core, requests in the open message, position) and
 * limit, every core's cycle and streaming position and, for PU_STREAM_SHARED_UNIFORM,
 * the re-use ring with its counters.  Without reseeding (reseed == 0; seeds == NULL) the
 * per-core generator states are copied too and the destination continues the source's
 * stream byte for byte.  With reseeding core k's generator state becomes seed * 2^32 + k,
 * the state a stream opened with that seed starts from, and the destination's seed
 * parameter becomes seed; nothing else changes.  So a fork at position 0 is the fresh
 * stream of the new seed, and positions and max_requests go on counting from the source's
 * position.  pu_dstream_fork: streams [first, first + n) of the set from stream src of
 * the same set, seeds[i] (host memory) for stream first + i; src inside the range is left
 * as it is and its entry ignored; asynchronous on hip_stream and ordered with the set's
 * other calls like pu_dstream_next.  A destination whose parameters differ from the
 * source's in any field but the seed is refused with PU_EINVAL and a message naming the
 * stream (its arrays are sized for its own shape), on the host, before anything is
 * launched or changed.  pu_stream_fits_req16 does not depend on the seed, so a set's
 * format-16 verdict stands.  PU_EINVAL for a NULL stream or set or a negative argument,
 * PU_ERANGE for src or the range outside the set. */
#define PU_FORK_BY_COPIES 1   /* the same result by one device-to-device copy per destination */
int pu_replica_fork(pu_handle* h, int src, int first, int n, int flags, void* hip_stream);
int pu_stream_fork(pu_stream* dst, const pu_stream* src, int reseed, uint64_t seed);
int pu_dstream_fork(pu_dstream* s, int src, int first, int n, const uint64_t* seeds, void* hip_stream);

/* One recorded trace replayed across an ensemble, placed per replica on the device (no
 * reference counterpart; the recorded-trace counterpart of pu_dstream_*: pu_dtrace_next ->
 * pu_run_device / _sliced / _pool -> pu_dsum_add, with the trace on the device once and no
 * request staged from the host).  Every replica of a handle shares one configuration, so
 * replicas of one trace are copies of one answer until something distinguishes them.  Two
 * things do, both a rewrite of two fields of each record:
 *   placement  a bijection of the trace's cores onto the configuration's, per replica: the
 *              thread-placement study of a NoC or a shared cache;
 *   skew       a constant added to the timers of each core, per replica: a sample of the
 *              interleavings a multi-threaded run could have taken.
 * A placement acts on the core ids a recorded trace already holds (pu_msglog_next has
 * resolved them).  The per-replica thread schedulers (pu_alloc_core_replica) are the other
 * end: they resolve (program, thread) to a core for the drop-in path, one request at a time.
 *
 * The rule (primesim_amd/csrc/trace_place_step.h), for a source record q of a replica with
 * placement row `place` and skew row `skew` (int32[num_cores] each; NULL = identity / zeros):
 *   core'  = place[q.core]
 *   timer' = q.timer + skew[q.core]           (indexed by the trace's core, not the placed one)
 *   addr, prog_id, mem_type, batch_start and tag are unchanged.
 * As pu_req (PU_REQ_FMT_32) all 32 bytes are written, _pad1 = 0 and tag copied; as pu_req16
 * (PU_REQ_FMT_16) the record is pu_pack_req16 of that 32-byte result.
 *
 * pu_dtrace_open: a set of `count` replicas over trace[0, n), whose cores lie in
 * [0, num_cores), with placement and skew as [count][num_cores] arrays (either may be NULL).
 * The trace is copied to `device` once and shared by all replicas; the rows are copied as
 * they are (32 B per record, 4 B per core, replica and table given).  Everything is checked
 * on the host before a device is touched; NULL + pu_last_error() on failure:
 *   PU_EINVAL  no trace, n == 0, count <= 0, num_cores outside 1 .. 65536;
 *   PU_ERANGE  a record whose core is outside [0, num_cores), naming the record;
 *   PU_EINVAL  a placement row that is no permutation of [0, num_cores), naming the replica
 *              and the first entry that is out of range or repeats an earlier one;
 *   PU_EINVAL  a negative skew, naming the replica and the core;
 *   PU_ERANGE  the largest timer plus the largest skew overflows int64;
 *   then "no HIP device" where there is none, as pu_create, and PU_ENOMEM with the size asked
 *   for when the device memory cannot be had.
 * The set fits pu_req16 when the largest timer plus the largest skew is below 2^40, no timer
 * is negative, every prog_id is in [0, 64), mem_type and batch_start are at most 1 and tag
 * is 0 (a placed core is below 65536 by construction): what pu_pack_req16 asks of every
 * placed record, decided once at open from the maxima, so it may refuse a set whose largest
 * timer and largest skew never meet.  pu_dtrace_fits_req16: 0, or PU_ERANGE with the reason.
 *
 * pu_dtrace_next: the contract of pu_dstream_next with one cursor for the whole set:
 * got = min(n_each, n - position); replica i's records [position, position + got) are placed
 * by replica i's rows and written to d_out[i*stride .. i*stride + got) (indices in records of
 * the chosen format; offsets are 64-bit); nothing else is written; d_got (device, count
 * uint64, may be NULL) receives got for every replica; the position advances by got.
 * stride >= n_each and d_out 16-byte aligned, else PU_EINVAL; PU_REQ_FMT_16 on a set that
 * does not fit: PU_ERANGE with the reason, before anything is launched (PU_REQ_FMT_32 still
 * serves that set).  Asynchronous on hip_stream (NULL = the set's own stream) and ordered
 * with the set's other calls as for pu_dstream_next.
 *
 * pu_dtrace_seek moves the cursor (0 <= position <= n, else PU_ERANGE; seek(0) replays the
 * trace) and pu_dtrace_position returns it (or PU_E*); both wait only for the set's
 * outstanding calls, never for the device, for the reason given for pu_dstream_* above.
 * pu_dtrace_state_bytes: device memory the set holds.  A NULL set: PU_EINVAL, 0, no-op.
 *
 * pu_trace_place: the same rule on host arrays, one replica's rows at a time (no device):
 * out holds n pu_req or n pu_req16 records.  It checks num_cores, the rows and every
 * record's core as pu_dtrace_open does, a timer plus skew that overflows int64 (PU_ERANGE),
 * and for PU_REQ_FMT_16 stops with PU_ERANGE at the first placed record that pu_pack_req16
 * would refuse, naming it (out untouched past it).
 *
 * pu_placement_shuffle: a placement row drawn from a seed, the same for every caller: the
 * identity for seed 0; otherwise the identity shuffled by Fisher-Yates from the top: for
 * i = num_cores - 1 down to 1, row[i] is swapped with row[j], j = draw mod (i + 1), the draws
 * being the splitmix64 sequence of the stream generators started at state `seed`
 * (z = (state += 0x9E3779B97F4A7C15); z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; draw = z ^ z >> 31).  PU_EINVAL for a NULL row or
 * num_cores outside 1 .. 65536. */
typedef struct pu_dtrace pu_dtrace;
pu_dtrace* pu_dtrace_open(const pu_req* trace, size_t n, int num_cores, int count,
                          const int32_t* placement /* [count][num_cores] or NULL */,
                          const int32_t* skew      /* [count][num_cores] or NULL */, int device);
void     pu_dtrace_close(pu_dtrace* s);
int      pu_dtrace_next(pu_dtrace* s, void* d_out, size_t n_each, size_t stride, int fmt,
                        uint64_t* d_got, void* hip_stream);
int      pu_dtrace_seek(pu_dtrace* s, int64_t position);
int64_t  pu_dtrace_position(pu_dtrace* s);
int      pu_dtrace_fits_req16(const pu_dtrace* s);
uint64_t pu_dtrace_state_bytes(const pu_dtrace* s);
int pu_trace_place(const pu_req* in, size_t n, const int32_t* place_row, const int32_t* skew_row,
                   int num_cores, int fmt, void* out);
int pu_placement_shuffle(int32_t* row, int num_cores, uint64_t seed);

/* Log-linear delay histograms kept on the device (no reference counterpart; a stage beside
 * pu_dsum_add on the same stream: pu_dstream_next -> pu_run_device -> pu_dsum_add ->
 * pu_dhist_add).  The 32 power-of-two buckets of pu_dsum_replica place a quantile within a
 * factor of two; these place it within 3.2 %, and exactly below 64 cycles, still without a
 * delay on the host.  Every figure is an exact integer and independent of the order of the
 * records, so the device result equals the host fold (pu_dhist_host_add) bit for bit, and
 * histograms add elementwise: chunks, replicas and ranks sum what they read.
 *
 * The rule (primesim_amd/csrc/delay_hist_step.h):
 *   class     as for pu_dsum_*: 0 = read, 1 = write (pu_req: mem_type == PU_WR).
 *   bucket    of a delay d (int32): 0 for d <= 0 (the meaning of pu_dsum's bucket 0); d itself
 *             for 1 <= d < 64; otherwise, with o = 31 - clz(d) (6 .. 30),
 *             64 + (o - 6) * 32 + ((d >> (o - 5)) - 32): every octave in 2^PU_DHIST_SUB_BITS
 *             equal parts.  INT32_MAX is in bucket 863 = PU_DHIST_BUCKETS - 1.  Buckets 1 .. 863
 *             tile [1, 2^31 - 1]; from bucket 64 on a bucket's width is <= its lower bound / 32.
 *   bounds    bucket 0 is [INT32_MIN, 0]; bucket k < 64 is [k, k]; bucket k >= 64, with
 *             j = k - 64, o = 6 + j / 32, m = 32 + j % 32: [m << (o - 5), ((m + 1) << (o - 5)) - 1].
 *   coarse    every fine bucket lies inside one bucket of pu_dsum_class.hist: 0 -> 0, k < 64 ->
 *             32 - clz(k), k >= 64 -> 7 + (k - 64) / 32.
 *   layout    uint64_t hist[2][PU_DHIST_BUCKETS] per replica (13,824 B); a class's count is the
 *             sum of its buckets.
 *   quantile  nearest rank.  A quantile is given in parts per million, ppm in [0, 1,000,000];
 *             rank = max(1, ceil(count * ppm / 10^6)), computed exactly through the 128-bit
 *             product; the answer is the lowest bucket whose inclusive running count reaches
 *             rank, or -1 for an empty class.  ppm 0 answers the minimum's bucket, 10^6 the
 *             maximum's.
 *
 * pu_dhist_open: `count` replicas on `device`; 13,824 B of device memory per replica plus the
 * quantile records and the slabs of the ensemble total.  NULL + pu_last_error() on failure
 * ("no HIP device" where there is none: the set has no CPU fallback; PU_ENOMEM with the size
 * asked for).
 *
 * pu_dhist_add: replica r counts the delays of records [d_begin[r], d_end[r]) into its
 * histogram; the arguments, their checks (d_reqs 16-byte aligned) and the ordering are
 * pu_dsum_add's, so one pair of index arrays serves both calls.
 *
 * pu_dhist_read: the histograms of replicas [first, first + n), 2 * PU_DHIST_BUCKETS
 * counters each.  pu_dhist_quantiles: for replicas [first, first + n) and both classes, the
 * class's count and the bucket of each of the nq (1 .. PU_DHIST_MAX_Q) quantiles ppm[0 .. nq),
 * formed on the device: out holds 2 * n records, [replica][class]; bucket[q] is -1 for q >= nq.
 * pu_dhist_read_total: the histogram summed over replicas [first, first + n) (2 *
 * PU_DHIST_BUCKETS counters; all zero for n = 0), formed when read by two launches without
 * atomics on the set's own stream.  pu_dhist_reset: every counter back to zero.
 * pu_dhist_state_bytes: device memory the set holds.  Reading, resetting and closing wait
 * only for the work of this set (the event of its last call), never for the device.
 * A NULL set: PU_EINVAL, 0, no-op; first < 0, n < 0, nq outside 1 .. PU_DHIST_MAX_Q or a ppm
 * above 10^6: PU_EINVAL; first + n > count: PU_ERANGE.
 *
 * Host twins, no device needed.  pu_dhist_host_add: n records added to hist
 * (uint64_t [2][PU_DHIST_BUCKETS], zeroed by the caller).  pu_dhist_host_quantiles: one class's
 * histogram (PU_DHIST_BUCKETS counters), its count to *count_out (may be NULL) and nq buckets
 * to bucket_out.  pu_dhist_bucket_of: the bucket of a delay.  pu_dhist_bucket_bounds: the
 * delays a bucket holds, both ends inclusive; PU_ERANGE for a bucket outside 0 .. 863. */
#define PU_DHIST_SUB_BITS 5
#define PU_DHIST_BUCKETS  864
#define PU_DHIST_MAX_Q    8
typedef struct pu_dhist_quantile {
    uint64_t count;                     /* records of the class */
    int32_t  bucket[PU_DHIST_MAX_Q];    /* per quantile asked for; -1: empty class, or not asked */
} pu_dhist_quantile;                    /* 40 bytes */

typedef struct pu_dhist pu_dhist;
pu_dhist* pu_dhist_open(int count, int device);
void      pu_dhist_close(pu_dhist* s);
int       pu_dhist_add(pu_dhist* s, const void* d_reqs, int fmt, const int32_t* d_delay,
                       const uint64_t* d_begin, const uint64_t* d_end, void* hip_stream);
int       pu_dhist_read(pu_dhist* s, int first, int n, uint64_t* out);
int       pu_dhist_quantiles(pu_dhist* s, int first, int n, const uint32_t* ppm, int nq,
                             pu_dhist_quantile* out);
int       pu_dhist_read_total(pu_dhist* s, int first, int n, uint64_t* out);
int       pu_dhist_reset(pu_dhist* s);
uint64_t  pu_dhist_state_bytes(const pu_dhist* s);
int       pu_dhist_host_add(uint64_t* hist, const void* reqs, int fmt, const int32_t* delays, size_t n);
int       pu_dhist_host_quantiles(const uint64_t* hist_one_class, const uint32_t* ppm, int nq,
                                  uint64_t* count_out, int32_t* bucket_out);
int       pu_dhist_bucket_of(int32_t d);
int       pu_dhist_bucket_bounds(int bucket, int32_t* lo, int32_t* hi);

/* Every replica's slowest requests kept on the device (no reference counterpart; one more
 * stage on the same stream: ... -> pu_dsum_add -> pu_dhist_add -> pu_dtail_add).  The
 * histograms say how large the tail is; these lists say which requests it is made of: core,
 * address, issue time and place in the stream of the K worst reads and the K worst writes of
 * every replica, still without a request or a delay on the host.  Every figure is an exact
 * integer and depends only on the concatenation of what was added, so the device result
 * equals the host fold (pu_dtail_host_add) bit for bit however the records were split into
 * calls.
 *
 * The rule (primesim_amd/csrc/delay_tail_step.h):
 *   set       `count` replicas and a list length k, 1 <= k <= PU_DTAIL_MAX_K, fixed at open.
 *   class     as for pu_dsum_*: 0 = read, 1 = write (pu_req: mem_type == PU_WR).
 *   seen      per replica, the records added since open or reset, both classes together.
 *   position  adding [begin, end) gives record i the position seen + (i - begin), then
 *             raises seen by end - begin; begin >= end adds nothing.
 *   order     entry x is better than entry y when x.delay > y.delay, or at equal delays when
 *             x.position < y.position.  Positions of a replica are distinct: a strict total
 *             order.  Delays of 0, negative delays and INT32_MIN are ordinary values.
 *   list      per replica and class the best min(k, records of the class seen) entries, best
 *             first; the entries past that count are all-zero bytes.
 *   total     the best k entries over replicas [first, first + n), per class, by delay
 *             descending, then replica ascending, then position ascending.
 *
 * pu_dtail_open: `count` replicas with lists of k entries on `device`; 64 * k + 16 B of device
 * memory per replica plus the partial lists of the ensemble total.  NULL + pu_last_error() on
 * failure (count < 1 or k outside 1 .. PU_DTAIL_MAX_K: before a device is touched; "no HIP
 * device" where there is none: the set has no CPU fallback).
 *
 * pu_dtail_add: replica r adds records [d_begin[r], d_end[r]); the arguments, their checks
 * (d_reqs 16-byte aligned) and the ordering are pu_dsum_add's and pu_dhist_add's, so one pair
 * of index arrays serves all three calls.  The request array is read again only for the
 * entries that enter a list.
 *
 * pu_dtail_read: the lists of replicas [first, first + n): out holds n * 2 * k entries,
 * [replica][class][rank], count_out n * 2 counts.  pu_dtail_read_total: the ensemble total of
 * replicas [first, first + n), formed when read by two launches without atomics on the set's
 * own stream: out holds 2 * k entries, replica_out the replica of each (-1 past the count),
 * count_out two counts; n = 0 gives empty lists.  pu_dtail_reset: every list empty and every
 * seen 0, the state after open.  pu_dtail_state_bytes: device memory the set holds.
 * pu_dtail_k: the list length (0 for NULL).  Reading, resetting and closing wait only for the
 * work of this set.  A NULL set: PU_EINVAL, 0, no-op; first < 0, n < 0 or a NULL output with
 * n > 0: PU_EINVAL; first + n > count: PU_ERANGE.
 *
 * Host twin, no device needed.  pu_dtail_host_add: n records added to one replica's lists
 * (entries [2][k], counts [2] and *seen, all zeroed by the caller before the first call). */
#define PU_DTAIL_MAX_K 64
typedef struct pu_dtail_entry {
    uint64_t addr;      /* pu_req.addr / pu_req16.a */
    int64_t  timer;     /* the recorded timer (pu_req.timer / PU_REQ16_TIMER) */
    uint64_t position;  /* as above */
    int32_t  delay;
    int32_t  core;      /* pu_req.core as it stands / PU_REQ16_CORE; not range-checked */
} pu_dtail_entry;       /* 32 bytes */

typedef struct pu_dtail pu_dtail;
pu_dtail* pu_dtail_open(int count, int k, int device);
void      pu_dtail_close(pu_dtail* s);
int       pu_dtail_add(pu_dtail* s, const void* d_reqs, int fmt, const int32_t* d_delay,
                       const uint64_t* d_begin, const uint64_t* d_end, void* hip_stream);
int       pu_dtail_read(pu_dtail* s, int first, int n, pu_dtail_entry* out /*[n][2][k]*/,
                        uint32_t* count_out /*[n][2]*/);
int       pu_dtail_read_total(pu_dtail* s, int first, int n, pu_dtail_entry* out /*[2][k]*/,
                              int32_t* replica_out /*[2][k]*/, uint32_t* count_out /*[2]*/);
int       pu_dtail_reset(pu_dtail* s);
uint64_t  pu_dtail_state_bytes(const pu_dtail* s);
int       pu_dtail_k(const pu_dtail* s);
int       pu_dtail_host_add(pu_dtail_entry* entries /*[2][k]*/, uint32_t* counts /*[2]*/, uint64_t* seen,
                            int k, const void* reqs, int fmt, const int32_t* delays, size_t n);

/* Every replica's delays over simulated time kept on the device (no reference counterpart;
 * one more stage on the same stream: ... -> pu_dsum_add -> pu_dhist_add -> pu_dtail_add ->
 * pu_dseries_add).  The summaries, histograms and lists fold a replica's whole measured
 * range into one figure; these series say when: per replica, class and epoch of the records'
 * own timers the count, the exact sum, the largest delay and the number of non-positive
 * delays, still without a request or a delay on the host.  At which cycle an open-loop
 * replica's delays start to climb, where it halted, how long a warm-up lasts: a user divides
 * sum by count per epoch.  Every figure is an exact integer and independent of the order of
 * the records, so the device result equals the host fold (pu_dseries_host_add) bit for bit,
 * and cells merge fieldwise: chunks, replicas and ranks add what they read (max: the larger).
 *
 * The rule (primesim_amd/csrc/delay_series_step.h):
 *   set       `count` replicas, E epochs (1 <= E <= PU_DSERIES_MAX_EPOCHS), a first cycle t0
 *             (any int64) and a shift (0 .. 62), fixed at open.  An epoch is 2^shift cycles.
 *   class     as for pu_dsum_*: 0 = read, 1 = write (pu_req: mem_type == PU_WR).
 *   timer     the record's own: pu_req.timer, or PU_REQ16_TIMER(b) of a pu_req16.
 *   epoch     0 for timer < t0; otherwise min(((uint64_t)timer - (uint64_t)t0) >> shift, E - 1).
 *             The distance is taken unsigned, so INT64_MAX against t0 = INT64_MIN is defined.
 *             The first and the last epoch are catch-alls: no record is dropped, and a
 *             replica's cells add up to what pu_dsum_* reports for the same records.
 *   cell      count: the records; sum: of every delay, non-positive ones included; nonpos: the
 *             delays <= 0 (the zeros a halted replica's remaining range reads, the -1 of a core
 *             id out of range, wrapped delays: what pu_dsum's bucket 0 counts); max: the
 *             largest of max(delay, 0).  An empty cell is all-zero bytes.
 *   layout    pu_dseries_cell cells[2][E] per replica (64 E bytes).
 *   total     the cells of replicas [first, first + n) merged: count, sum and nonpos added,
 *             max the largest.
 *
 * pu_dseries_open: `count` replicas with E epochs on `device`; 64 E bytes of device memory per
 * replica plus the slabs of the ensemble total.  NULL + pu_last_error() on failure (count < 1,
 * epochs outside 1 .. PU_DSERIES_MAX_EPOCHS or shift outside 0 .. 62: before a device is
 * touched; "no HIP device" where there is none: the set has no CPU fallback).
 *
 * pu_dseries_add: replica r folds records [d_begin[r], d_end[r]) into its cells; the
 * arguments, their checks (d_reqs 16-byte aligned) and the ordering are pu_dsum_add's, so one
 * pair of index arrays serves all four calls.
 *
 * pu_dseries_read: the cells of replicas [first, first + n): out holds n * 2 * E cells,
 * [replica][class][epoch].  pu_dseries_read_total: the ensemble total of replicas
 * [first, first + n) (2 * E cells; all zero for n = 0), formed when read by two launches
 * without atomics on the set's own stream.  pu_dseries_reset: every cell back to zero.
 * pu_dseries_state_bytes: device memory the set holds.  pu_dseries_epochs: E (0 for NULL).
 * Reading, resetting and closing wait only for the work of this set.  A NULL set: PU_EINVAL,
 * 0, no-op; first < 0, n < 0 or a NULL output with n > 0: PU_EINVAL; first + n > count:
 * PU_ERANGE.
 *
 * Host twins, no device needed.  pu_dseries_host_add: n records folded into one replica's
 * cells ([2][epochs], zeroed by the caller before the first call).  pu_dseries_epoch_of: the
 * epoch of a timer; PU_EINVAL for epochs or shift out of range. */
#define PU_DSERIES_MAX_EPOCHS 512
typedef struct pu_dseries_cell {
    uint64_t count;     /* records of the class in the epoch */
    int64_t  sum;       /* of every delay */
    uint64_t nonpos;    /* delays <= 0 */
    int32_t  max;       /* the largest of max(delay, 0) */
    int32_t  _pad;
} pu_dseries_cell;      /* 32 bytes */

typedef struct pu_dseries pu_dseries;
pu_dseries* pu_dseries_open(int count, int epochs, int64_t t0, int shift, int device);
void        pu_dseries_close(pu_dseries* s);
int         pu_dseries_add(pu_dseries* s, const void* d_reqs, int fmt, const int32_t* d_delay,
                           const uint64_t* d_begin, const uint64_t* d_end, void* hip_stream);
int         pu_dseries_read(pu_dseries* s, int first, int n, pu_dseries_cell* out /*[n][2][E]*/);
int         pu_dseries_read_total(pu_dseries* s, int first, int n, pu_dseries_cell* out /*[2][E]*/);
int         pu_dseries_reset(pu_dseries* s);
uint64_t    pu_dseries_state_bytes(const pu_dseries* s);
int         pu_dseries_epochs(const pu_dseries* s);
int         pu_dseries_host_add(pu_dseries_cell* cells /*[2][epochs]*/, int epochs, int64_t t0, int shift,
                                const void* reqs, int fmt, const int32_t* delays, size_t n);
int         pu_dseries_epoch_of(int64_t timer, int epochs, int64_t t0, int shift);

/* Trace files ("PUTRACE1": header, thread table, pu_req records). */
int pu_trace_write(const char* path, const pu_req* reqs, size_t n,
                   const int32_t* thread_prog, const int32_t* thread_id, int num_threads);

/* ------------------------------------------------------------------------
 * MsgMem message logs: the receive stream of the
 * reference's uncore server, message by message as prime.cpp:53 gets it
 * (MPI source rank + the MsgMem records of reference src/common.h:49-59, 24 B
 * each).  File: "PRIMEMSG" | u32 1 | u32 24, then per message
 * i32 source | i32 n_records | records.  Replay applies prime.cpp:55-137:
 * NEW_THREAD -> allocCore, THREAD_FINISHING -> deallocCore, MEM_REQUESTS ->
 * getCoreId + requests 1..addr_dmem-1 with prog_id = source; other control
 * messages have no uncore effect, PROGRAM_EXITING ends the log.
 * ---------------------------------------------------------------------- */
typedef struct pu_msglog pu_msglog;
/* Open for replay; num_cores sizes the log's own ThreadSched (used when
 * pu_msglog_next gets h == NULL). */
pu_msglog* pu_msglog_open(const char* path, int num_cores);
/* Next requests (<= cap) in receive order, core ids resolved through h's
 * ThreadSched (h may be NULL: the log's own).  batch_start marks each
 * message's first request.  Returns the count, 0 at the end, or PU_E*. */
int64_t    pu_msglog_next(pu_msglog* L, pu_handle* h, pu_req* out, size_t cap);
int64_t    pu_msglog_messages(const pu_msglog* L);
/* Capture: create a log and append messages as received (the three fwrite
 * calls a prime.cpp build would add after MPI_Recv). */
pu_msglog* pu_msglog_create(const char* path);
int        pu_msglog_append(pu_msglog* L, int32_t source, const void* records, int32_t n_records);
int        pu_msglog_close(pu_msglog* L);
/* A canonical-order request stream written as the log its cores would have
 * sent (NEW_THREAD per thread, one MEM_REQUESTS message per batch). */
int pu_msglog_from_requests(const char* path, const pu_req* reqs, size_t n, const int32_t* thread_prog,
                            const int32_t* thread_id, int num_threads, const int32_t* core_thread,
                            int num_cores);

/* ------------------------------------------------------------------------
 * Server front-end: prime.cpp's message loop
 * (reference src/prime.cpp:35-137, main :142-233) behind a Unix-domain socket
 * instead of MPI, feeding the engine a round at a time.
 *
 * A session is one simulation (one prime.cpp process in the reference) and
 * runs on one replica; its clients are the Pin processes of that simulation,
 * identified by their rank (the MPI source, = prog_id).  Clients exchange
 * exactly what core_manager.cpp sends and receives over MPI: MsgMem buffers
 * (24-B records, common.h:49-59) sent with a tag, and int replies received
 * on a tag (pu_client_*; INTEGRATION.md shows the core_manager.cpp edit).
 * Every message is handled with prime.cpp's rules: PROCESS_STARTING /
 * PROCESS_FINISHING / INTER_PROCESS_BARRIERS maintain the program list and
 * release barriers (replies on tag 0), NEW_THREAD allocates a core (reply
 * core % num_recv_threads on tag thread), THREAD_FINISHING frees it,
 * MEM_REQUESTS runs requests 1..msg[0].addr_dmem-1 with the running delay of
 * prime.cpp:129 (reply: the batch delay on tag thread), PROGRAM_EXITING ends
 * one handler thread; a session ends after num_recv_threads of them and
 * writes its report (UncoreManager::report) to <report_prefix>_<session>.
 * A negative batch delay stops that message's receive thread like
 * prime.cpp:130-134 (its handler returns): the message gets no reply, later
 * messages on its tag are never received, and once every receive thread has
 * returned the report is written and the session's connections are closed.
 * An engine limit (PU_ERRF_LIMITS) ends the session with an error instead of
 * replying with delays that are no longer the reference's.
 *
 * Rounds: each round reads everything the clients have sent, takes from every
 * session its pending messages up to the first control message that follows
 * a MEM_REQUESTS message (so control messages never overtake a batch whose
 * outcome could stop the session), and runs all sessions' MEM_REQUESTS
 * batches in ONE engine launch (pu_run_device: one wavefront per session),
 * then sends the replies.  Per session the result is the sequential one of
 * prime.cpp with one receive thread, in the order the server received the
 * messages.
 * ---------------------------------------------------------------------- */
typedef struct pu_server pu_server;

typedef struct pu_server_opts {
    const char* socket_path;   /* Unix-domain socket path to listen on */
    const char* report_prefix; /* session s writes <prefix>_<s> when it ends; NULL = no file */
    int num_sessions;          /* sessions 0..n-1 (<= replicas); run() returns when all have ended */
    int num_recv_threads;      /* XmlSim::num_recv_threads (prime.cpp:182); 0 = 1 */
    int max_msg_size;          /* XmlSim::max_msg_size: records per message beyond the header; 0 = 100 */
    int verbose;               /* print prime.cpp's "[PriME] ..." progress lines */
} pu_server_opts;

typedef struct pu_server_stats {
    uint64_t rounds;           /* service rounds that handled at least one message */
    uint64_t launches;         /* engine launches (rounds with MEM_REQUESTS) */
    uint64_t messages;         /* MsgMem messages handled */
    uint64_t requests;         /* memory requests sent to the engine */
    int32_t  sessions_ended;
    int32_t  sessions_halted;  /* a receive thread stopped by a negative batch delay */
    int32_t  sessions_failed;  /* ended by an engine limit (PU_ERRF_LIMITS): no exact reply possible */
    int32_t  _pad;
} pu_server_stats;

/* Host executor: runs one session's requests in order and writes each
 * request's uncore_access delay (the engine's per-request output).  Lets the
 * protocol be exercised without a GPU (tests); the product path is
 * pu_server_create on an engine handle.  Returns 0, a negative PU_E* (the
 * round fails), or positive PU_ERRF_* bits the session's replica now carries. */
typedef int (*pu_exec_fn)(void* ctx, int session, const pu_req* reqs, size_t n, int32_t* delays);

/* Serve engine handle h (not owned; sessions <= pu_num_replicas(h)). */
pu_server* pu_server_create(pu_handle* h, const pu_server_opts* o);
pu_server* pu_server_create_exec(pu_exec_fn fn, void* ctx, int num_cores, const pu_server_opts* o);
/* Serve until every session has ended or pu_server_stop (which ends this run;
 * calling pu_server_run again resumes serving); 0 or PU_E*. */
int  pu_server_run(pu_server* s);
/* One round, waiting up to timeout_ms for the first message; returns the
 * number of messages handled (>= 0) or PU_E*. */
int  pu_server_round(pu_server* s, int timeout_ms);
void pu_server_stop(pu_server* s);     /* thread-safe */
int  pu_server_get_stats(pu_server* s, pu_server_stats* out);
void pu_server_destroy(pu_server* s);

/* Client: the MPI calls of core_manager.cpp.  One client per Pin thread (or a
 * mutex around a shared one).  send = MPI_Send(records, n*24, MPI_CHAR, 0,
 * tag); recv = MPI_Recv(value, 1, MPI_INT, 0, tag) with MPI's matching (a
 * reply sent before the receive is posted waits at the server). */
typedef struct pu_client pu_client;
pu_client* pu_client_connect(const char* socket_path, int session, int rank);
int  pu_client_send(pu_client* c, int tag, const void* records, int n_records);
int  pu_client_recv(pu_client* c, int tag, int32_t* value);
void pu_client_close(pu_client* c);

/* ------------------------------------------------------------------------
 * Unit hooks: run one engine component alone on the GPU (one wavefront), for
 * the component-level parity tests.
 * ---------------------------------------------------------------------- */
/* QueueModelHistoryTree::computeQueueDelay sequence on a fresh queue
 * (queue_model_history_tree.cpp:42-125 + queue_model_m_g_1.cpp). */
int pu_unit_queue_run(uint64_t min_proc, const uint64_t* t, const uint64_t* p, size_t n,
                      uint64_t* delay_out, uint64_t* mg1_calls, int device);
/* QueueModelMG1::computeQueueDelay (queue_model_m_g_1.cpp:16-42) evaluated by
 * the engine's M/G/1 arithmetic on n given queue states: state i is
 * _num_arrivals = num_arrivals[i] (< 2^53), _sigma_service_time = sum[i],
 * _sigma_service_time_square = sum_sq[i], _newest_arrival_time = newest[i];
 * wait_out[i] = the queue delay.  The arithmetic fuzz of the M/G/1 branch. */
int pu_unit_mg1_run(const uint64_t* num_arrivals, const double* sum, const double* sum_sq,
                    const uint64_t* newest, size_t n, uint64_t* wait_out, int device);
/* The same, and which way the arithmetic went: path_out[i] = 1 when the
 * one-division closed form was proven to give the reference's wait (its guard
 * held), 0 when the reference's own five-division chain ran. */
int pu_unit_mg1_path_run(const uint64_t* num_arrivals, const double* sum, const double* sum_sq,
                         const uint64_t* newest, size_t n, uint64_t* wait_out, uint8_t* path_out,
                         int device);
/* Network::transmit sequence on a fresh mesh (network.cpp:97-160); st gets
 * the network counters. */
int pu_unit_network_run(int num_nodes, int net_type, int data_width, int header_flits,
                        uint64_t router_delay, uint64_t link_delay, uint64_t inject_delay,
                        const int32_t* src, const int32_t* dst, const int32_t* len,
                        const uint64_t* timer, size_t n, uint64_t* delay_out, pu_stats* st,
                        int device);

#ifdef __cplusplus
}
#endif
#endif /* PRIMEUNCORE_H */
