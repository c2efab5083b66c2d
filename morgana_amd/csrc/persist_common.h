// Shared pieces of the persistent (one launch for all time steps) recurrent kernels: group / slot geometry, the workspace layout,
// the flag hand-off helpers, the XCD detection, the kernels' common first lines, the time-out codes and the entry points' launch
// set-up.  Protocol and measurements: gru_persist.hip (header comment), DESIGN.md section 4.
#pragma once

#include "common.h"

#define GT 16
#define GP_GROUPS 8
#define GP_SLOTS 32                          // flag words per group (H <= 512)
#define GP_KSTEPS 4                          // H / 128 MFMA k-steps per wave, H <= 512
#define GP_SPIN_LIMIT (1u << 22)              // polls before a wait gives up (a poll is 0.2-0.5 us: 1-2 s)
#define GP_TICKET_OFFSET (2 * GP_GROUPS * GP_SLOTS) // slot tickets, one counter per group (gp_claim_slot)
#define GP_FLAG_WORDS (GP_TICKET_OFFSET + GP_GROUPS) // per launch (zeroed by a memset node): step flags [8][32], XCC ids [8][32], tickets [8]
#define GP_SYNC_WORDS (GP_FLAG_WORDS + 4)          // + {sticky status, 3 pad}: 2096 bytes, a multiple of 16

typedef __bf16 gbf8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned gu32;

__device__ __forceinline__ gbf8 as_bf8(u32x4 v) {
    union { u32x4 u; gbf8 b; } c;
    c.u = v;
    return c.b;
}

// What a workgroup stores in the sticky status word (behind the flags; mg_gru_persist_status reports it) when one of its bounded waits
// gives up.  The values are quoted by logs of earlier runs: they stay, also where two kernels share one.
enum gp_status : unsigned {
    GP_ST_GRU_FWD = 1,         // gru_fwd_persist_kernel: the group's state flags of a step
    GP_ST_GRU_BWD = 2,         // gru_bwd_persist_kernel / gru_bwd_persist_wide_kernel: the group's gate-gradient flags of a step
    GP_ST_XCD = 3,             // any kernel: the XCD ids of the group's other slots (gp_one_xcd_or_report, before the first step)
    GP_ST_LSTM_FWD = 4,        // lstm_fwd_persist_kernel: the group's state flags of a step
    GP_ST_LSTM_BWD = 5,        // lstm_bwd_persist_kernel: the group's gate-gradient flags of a step
    GP_ST_LSTM_STACK_FWD = 6,  // lstm_stack_fwd_persist_kernel: own, lower or upper layer's flags of a step (lps_wait)
    GP_ST_LSTM_STACK_BWD = 7,  // lstm_stack_bwd_persist_kernel: either of its two waits of a step (lps_wait)
    GP_ST_GRU_FWD_F32 = 7,     // gru_fwd_persist_f32_kernel: the group's state flags of a step (the same number as the line above)
    GP_ST_GRU_BWD_F32 = 8,     // gru_bwd_persist_f32_kernel: the group's gate-gradient flags of a step
    GP_ST_GRU_STACK_FWD = 8,   // gru_stack_fwd_small64_kernel: the lower layer's output of a step (the same number as the line above)
    GP_ST_LSTM_FWD_F32 = 9,    // lstm_fwd_persist_f32_kernel: the group's state flags of a step
    GP_ST_GRU_STACK_BWD = 9,   // gru_stack_bwd_small64_kernel: the upper layer's input gradient of a step (the same number as the line above)
    GP_ST_LSTM_BWD_F32 = 10,   // lstm_bwd_persist_f32_kernel: the group's gate-gradient flags of a step
};

__device__ __forceinline__ void gp_report(gu32* status, gp_status code) {
    __hip_atomic_store(status, (unsigned)code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slot's flag: written through (sc1) in general; within one XCD a store that stays in the shared L2 (workgroup scope = no
// sc1 bit; the pollers' sc1 loads are L2-served)
__device__ __forceinline__ void gp_store_flag(gu32* flag, unsigned epoch, int one_xcd) {
    if (one_xcd)
        __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wave 0: wait until every slot's flag of the group has reached `epoch`.  Returns false after GP_SPIN_LIMIT polls.
__device__ __forceinline__ bool gp_wait_flags(gu32* flags, int n_slots, unsigned epoch, int lane) {
    for (unsigned spins = 0;; ++spins) {
        const unsigned f = lane < n_slots ? __hip_atomic_load(flags + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : epoch;
        if (__all(f >= epoch)) return true;
        if (spins > GP_SPIN_LIMIT) return false;
        __builtin_amdgcn_s_sleep(1);
    }
}

// Workgroup barrier for LDS hand-overs inside the step loops: waits for this wave's LDS operations only.  __syncthreads() also
// drains the wave's global stores (its release fence = s_waitcnt vmcnt(0)): the waves that write a step's fp32 results would
// then reach the next barrier a store round trip late, every step.
__device__ __forceinline__ void gp_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Which (group, slot) a workgroup serves.  HIP promises nothing about the block -> XCD map (MI355X_MICROARCH.md: observed round-robin
// dealing, "for speed only"), and a group whose slots sit on several XCDs pays the write-through hand-off on every one of its T
// steps (C4 5.5 instead of 3.4 ms).  So membership is not read off the block index: the workgroup reads the id of the XCD it finds
// itself on and takes a ticket of THAT id's group - as long as the launch puts n_slots workgroups on every XCD (one per CU: the
// usual case) every group is complete on one XCD whatever the dealing order was.  A workgroup whose XCD's group is already full
// (an over-subscribed XCD) takes a ticket of the next group that still has a slot: 8 groups x n_slots slots, exactly as many
// workgroups, every ticket below n_slots is a distinct slot - so every workgroup finds one within 8 atomics and every slot gets
// an owner (if all 8 groups were full, 8 n_slots OTHER workgroups would own slots: one more than exist).  A group that ends up
// with members on several XCDs is found by gp_group_on_one_xcd below and keeps the placement-independent write-through form.
// Returns group * GP_SLOTS + slot, or -1 for a workgroup beyond the 8 n_slots the launch needs.  The tickets are zeroed with the
// flags by the memset node ahead of the launch.
__device__ __forceinline__ int gp_claim_slot(gu32* tickets, int n_slots, int tid, int* s_word) {
    if (tid == 0) {
        unsigned id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(id));
        int got = -1;
        for (int a = 0; a < GP_GROUPS && got < 0; ++a) {
            const int g = (int)((id + (unsigned)a) % GP_GROUPS);
            const unsigned t = __hip_atomic_fetch_add(tickets + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t < (unsigned)n_slots) got = g * GP_SLOTS + (int)t;
        }
        *s_word = got;
    }
    __syncthreads();
    const int v = *s_word;
    __syncthreads();                                   // the caller reuses the word
    return v;
}

// Where the group runs.  Every workgroup publishes the id of the XCD it is on (s_getreg HW_REG_XCC_ID) and reads the ids of the
// group's other slots - once per launch, with the placement-independent sc1 protocol.  If they are all equal, the whole group
// shares one L2: the hand-off stores may then stay plain (the line stays in that L2, where the readers' sc1 loads - which only
// bypass their own CU's L1 - find it) instead of being written through to memory and fetched back over the fabric.  The
// block -> XCD map itself is never assumed: a group spread over several XCDs keeps the write-through form.
// Returns 1 = one XCD, 0 = several, -1 = timed out.
__device__ __forceinline__ int gp_group_on_one_xcd(gu32* xcc_tab, int slot, int n_slots, int tid, int* s_word) {
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(id));
    if (tid == 0) __hip_atomic_store(xcc_tab + slot, id + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {
        int result = -1;
        for (unsigned spins = 0; spins <= GP_SPIN_LIMIT; ++spins) {
            const unsigned v = tid < n_slots ? __hip_atomic_load(xcc_tab + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : id + 1u;
            if (__all(v != 0u)) {
                result = __all(v == id + 1u) ? 1 : 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (tid == 0) *s_word = result;
    }
    __syncthreads();
    return *s_word;
}

// The detection as the kernels use it: MG_TUNE_GRU_HANDOFF bit 0 skips it (0: the write-through form everywhere); a time-out is
// reported here and comes back as -1, on which the kernel returns.
__device__ __forceinline__ int gp_one_xcd_or_report(gu32* xcc_tab, int slot, int n_slots, int tid, int* s_word, int handoff, gu32* status) {
    const int one_xcd = (handoff & 1) ? 0 : gp_group_on_one_xcd(xcc_tab, slot, n_slots, tid, s_word);
    if (one_xcd < 0) {
        if (tid == 0) gp_report(status, GP_ST_XCD);
    }
    return one_xcd;
}

// A single-layer kernel's first lines: which (group, slot) the workgroup serves (a ticket, gp_claim_slot), the group's rows
// [row0, row0 + nrows) of the batch, its flag row, the status word, and whether the group sits on one XCD.  Clears *s_abort.
// !ok: the workgroup has nothing to do, or the detection timed out (reported): the kernel returns.
struct gp_place {
    int group, slot, row0, nrows, one_xcd;
    gu32 *flags, *status;
    bool ok;
};
__device__ __forceinline__ gp_place gp_enter(unsigned* sync, int n_slots, int B, int R, int handoff, int tid, int* s_abort, int* s_word) {
    gp_place p = {};
    const int claim = gp_claim_slot((gu32*)sync + GP_TICKET_OFFSET, n_slots, tid, s_word);
    if (claim < 0) return p;
    p.group = claim / GP_SLOTS;
    p.slot = claim % GP_SLOTS;
    p.row0 = p.group * R;
    p.nrows = min(R, B - p.row0);
    if (p.slot >= n_slots || p.nrows <= 0) return p;
    p.flags = (gu32*)sync + p.group * GP_SLOTS;
    p.status = (gu32*)sync + GP_FLAG_WORDS;
    if (tid == 0) *s_abort = 0;
    p.one_xcd = gp_one_xcd_or_report((gu32*)sync + GP_GROUPS * GP_SLOTS + p.group * GP_SLOTS, p.slot, n_slots, tid, s_word, handoff, p.status);
    p.ok = p.one_xcd >= 0;
    return p;
}

// Longest sequence among the group's rows (at most T): steps at or beyond it need no matmul and no hand-off.  (Two kernels keep this
// loop open-coded, and one gp_enter's lines: there the compiler allocates registers differently when they come from here.)
__device__ __forceinline__ int gp_longest(const int64_t* seq_len, int row0, int nrows, int T) {
    int gmax = 0;
    for (int r = 0; r < nrows; ++r) {
        const int64_t n = seq_len ? seq_len[row0 + r] : (int64_t)T;
        gmax = max(gmax, (int)(n < T ? n : T));
    }
    return gmax;
}

// Residency: every workgroup of a persistent launch must be on the device at once.  The kernels need up to 256 VGPRs, i.e. as
// few as two 256-thread workgroups per CU: a launch is offered only if the current device has room for `workgroups` at two
// per CU (MI355X: 256 CUs; a partitioned or harvested device simply takes the per-step kernels instead of timing out).
static inline int gp_device_holds(long workgroups) {
    static int cus = -1;
    if (cus < 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
        cus = n;
    }
    return cus > 0 && workgroups <= 2L * cus;
}

// workspace: [step flags 8 x 32 words | XCC ids 8 x 32 words | status word + 3 pad] [hand-off ring]
#define GP_RING_OFFSET ((size_t)GP_SYNC_WORDS * sizeof(unsigned))

// What every single-layer entry point does between its own argument checks and its launch: the workspace must be there, 16-byte
// aligned and large enough (mg_gru_persist_workspace_bytes); the flags, XCC ids and tickets are zeroed on the stream; then the
// launch geometry.  Returns MG_OK or the code the entry point returns (error text set).
struct gp_launch {
    int R;                 // items per group
    unsigned grid;         // workgroups: 8 groups x H / 16 slots
    void* ring;            // the hand-off ring behind the flags
    int handoff;           // MG_TUNE_GRU_HANDOFF
};
static inline int gp_prepare_launch(const char* what, int B, int H, void* workspace, size_t workspace_bytes, hipStream_t st, gp_launch* l) {
    MG_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "%s: workspace must be 16-byte aligned", what);
    if (!workspace || workspace_bytes < mg_gru_persist_workspace_bytes(B, H)) {
        mg_set_error("%s: workspace of %zu bytes needed, got %zu", what, mg_gru_persist_workspace_bytes(B, H), workspace_bytes);
        return MG_EWORKSPACE;
    }
    if (hipMemsetAsync(workspace, 0, (size_t)GP_FLAG_WORDS * sizeof(unsigned), st) != hipSuccess) {
        mg_set_error("%s: memset failed", what);
        return MG_ELAUNCH;
    }
    l->R = (int)mg_ceil_div(B, GP_GROUPS);
    l->grid = (unsigned)(GP_GROUPS * (H / GT));
    l->ring = (char*)workspace + GP_RING_OFFSET;
    l->handoff = g_mg_tuning[MG_TUNE_GRU_HANDOFF];
    return MG_OK;
}
