// kss_simple.cuh — the sequential scheduling loop for batches without PodTopologySpread /
// InterPodAffinity programs (the default-profile workload of BASELINE C1/C2/C5), built
// around ONE cross-shard exchange per pod.
//
// Same semantics as schedule_pod<false> (kss_sched.cuh), split in two kernels:
//
//   k_static  (massively parallel, one lane per (pod, node)): everything of a pod's
//             evaluation that no commit can change — the NodeUnschedulable, NodeName,
//             TaintToleration and NodeAffinity filters (node flags, taints and labels are
//             not touched by AssumePod) and the raw TaintToleration and NodeAffinity
//             scores — packed in one 32-bit "static word" per (pod, node) in HBM.
//   k_simple  (persistent, one workgroup per shard of W): the sequential loop.  Per pod it
//             only evaluates what the state changes: the NodeResourcesFit filter, the Fit
//             and BalancedAllocation scores (exact reciprocal arithmetic, kss_fastmath.cuh),
//             then NormalizeScore, the packed selectHost key and the commit.
//
// The persistent loop:
//   * the shard's node rows and their Allocatable reciprocals live in LDS for the launch;
//   * the compact pod records (SPod) and the static words of pod k+2 are loaded into
//     registers while pod k is scheduled and stored into 3-slot LDS rings at its end;
//   * pod k's argmax and pod k+1's normalisation statistics travel in the same exchange.
//     Pod k+1's statistics depend on pod k's commit, which touches one node only: the
//     winner, which is some shard's local best.  Each shard therefore evaluates pod k+1
//     on its local best node twice — before the commit (H0) and after it (H1) — and
//     publishes both statistic sets next to its pod-k key.  Once the global winner is
//     known, the winner's shard contributes H1 and every other shard H0, which is the
//     statistic of pod k+1 on the committed state.
#pragma once
#include "kss_fastmath.cuh"
#include "kss_sched.cuh"

namespace kss {

// Global-memory accesses of the persistent loop go through address-space-1 pointers:
// from a generic pointer the compiler emits flat instructions, which also count in
// lgkmcnt, so every LDS-only barrier (s_waitcnt lgkmcnt(0)) would wait for the HBM
// prefetches and the commit's atomics.
#define KSS_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ KSS_GLOBAL T* gp(T* p) {
  return (KSS_GLOBAL T*)p;
}

// Node state and static words handed from one launch to the next (k_static -> loop kernel,
// a chunk's write-back -> the next chunk's load, a reset copy -> the first load) go through
// agent-scope (sc1) stores and loads: the per-XCD L2s are not coherent with each other, and a
// line a workgroup of an earlier launch left in its XCD's L2 must not satisfy a later load on
// that XCD.  (Observed: a split-grid run reading one stale class count at a chunk boundary.)
// (through address-space-1 pointers: a flat access would also count in lgkmcnt, and every
// following LDS wait would then wait on it)
template <class T>
__device__ __forceinline__ T ld_ag(const T* p) {
  return __hip_atomic_load(gp(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ T ld_ag(KSS_GLOBAL const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ void st_ag(T* p, T v) {
  __hip_atomic_store(gp(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The ends of a launch-to-launch hand-off of node state (a chunk's write-back -> the next
// chunk's load, k_static -> the loop kernel, a reset / delta -> the next launch), in the
// producer / consumer forms of MI355X_MICROARCH.md ("Valid forms"): every storing wave
// waits for its own stores, then (after a workgroup barrier where the caller has one) an
// agent-scope release writes the XCD's L2 back; the consumer starts with an agent-scope
// acquire.  The kernel boundary alone did not order them under a concurrent split-grid part
// (DESIGN §5).
__device__ __forceinline__ void handoff_drain() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void handoff_release() {  // whole workgroup, no thread exited
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) handoff_drain();
}
__device__ __forceinline__ void handoff_acquire() {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__device__ __forceinline__ int xcc_id() {
  int x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  return x & 0xF;
}

// Publish one granule at offset `off` of the exchange buffer (the local inbox `gran`);
// address-space-1 stores (a flat store would also count in lgkmcnt).  An XCD-local grid
// (X.xcd_local: every shard runs on the same XCD, xcd_slot) publishes with a plain store (no
// cache-policy bits): the line stays in that XCD's L2, which every shard's agent-scope
// (L1-bypassing) poll reads -- a third of the latency of a write-through granule
// (tools/xcd_exchange_probe.hip, 32-way rounds: 0.41 against 1.23 us).
__device__ __forceinline__ void xpub(const XPeers& X, unsigned long long* gran, size_t off, unsigned long long v) {
  if (X.n <= 1) {
    if (X.xcd_local) asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(gran + off), "v"(v) : "memory");
    else __hip_atomic_store(gp(gran) + off, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  for (int p = 0; p < X.n; p++) __hip_atomic_store(gp(X.inbox[p]) + off, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int SX_VALS = 8;    // granules per shard per exchange: key lo/hi, H0 (nf, tt, na), H1 (nf, tt, na)

// An XCD-local k_simple grid (one cluster, W <= CUs per XCD): the launch has XCD_GRID_MULT x W
// workgroups; the first W that run on XCD 0 become shards 0 .. W-1 in arrival order and every
// other workgroup leaves at once.  Correctness never rests on where the hardware places a
// workgroup: a shard is one that READ its XCC id as 0, so all shards share XCD 0's L2.  When
// XCD 0 gets fewer than W of them (counted once every workgroup of the grid has started), the
// launch fails with err = 3 before touching any state and the host runs it again unrestricted.
// ctr: two zeroed words behind the launch's granules, [0] shards taken, [1] workgroups started.
// Returns the shard, -1 (leave), -2 (placement failed).  force_fail (kss_set_option
// "xcd_force_fallback", tests): workgroup 0 reports failed placement and every workgroup leaves,
// so the host's unrestricted rerun is what schedules the batch.
constexpr int XCD_GRID_MULT = 8;
__device__ __forceinline__ int xcd_slot(int* ctr, int W, int grid, int* err, bool force_fail = false) {
  if (force_fail) {
    if (blockIdx.x == 0) err_raise(err, 3);
    return blockIdx.x == 0 ? -2 : -1;
  }
  int slot = -1;
  if (xcc_id() == 0) {
    slot = atomicAdd(&ctr[0], 1);
    if (slot >= W) slot = -1;
  }
  atomicAdd(&ctr[1], 1);  // after the slot: every workgroup started => every XCD-0 slot taken
  if (slot < 0) return -1;
  long long t0 = 0;
  for (unsigned spins = 0;; ++spins) {
    if (__hip_atomic_load(&ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= W) return slot;
    if (__hip_atomic_load(&ctr[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= grid &&
        __hip_atomic_load(&ctr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < W)
      break;
    if (spin_expired(spins, t0)) break;
    __builtin_amdgcn_s_sleep(1);
  }
  err_raise(err, 3);
  return -2;
}
// The XCD-slot claim at the head of a loop kernel (k_simple, k_simple_tab, k_spread) on an XCD-local
// grid: thread 0 claims (xcd_slot), the workgroup learns the result through H.pad[0].  ctr_off():
// where the launch's two counters lie behind its granules, in granules (a callable: the claiming
// thread alone evaluates it).  Whole workgroup.  Returns xcd_slot's value: the shard, or < 0 (leave).
template <class Hdr, class CtrOff>
__device__ __forceinline__ int claim_xcd_shard(Hdr& H, const XPeers& X, unsigned long long* gran, CtrOff ctr_off, int W,
                                               int* err) {
  if (threadIdx.x == 0)
    H.pad[0] = xcd_slot(reinterpret_cast<int*>(gran + ctr_off()), W, (int)gridDim.x, err, X.xcd_local == 2);
  __syncthreads();
  return H.pad[0];
}
// A runtime (non-default) profile into the header's LDS copy (whole workgroup).
template <class Hdr>
__device__ __forceinline__ void stage_profile(Hdr& H, const kss_profile& from) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&from);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&H.prof);
  for (int i = threadIdx.x; i < (int)(sizeof(kss_profile) / 4); i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}
constexpr int SX_CHUNKS = 2;  // shards swept 64 at a time: W <= 128
constexpr int STATIC_PODS = 8;  // pods per k_static lane
constexpr int PF_MAX = 8;       // static words per prefetch lane (host-checked: simple_fits)

// The v1.26 default profile (kss_default_profile, kss_host.cpp; plugins_test.go:184-204,
// 878-1096) as a compile-time constant: k_simple<true> folds every weight and resource
// choice of the scoring path into the code.
__host__ __device__ constexpr kss_profile default_profile_c() {
  kss_profile p{};
  p.weight[KSS_S_TAINT_TOLERATION] = 3;
  p.weight[KSS_S_NODE_AFFINITY] = 2;
  p.weight[KSS_S_NODE_RESOURCES_FIT] = 1;
  p.weight[KSS_S_VOLUME_BINDING] = 1;
  p.weight[KSS_S_POD_TOPOLOGY_SPREAD] = 2;
  p.weight[KSS_S_INTER_POD_AFFINITY] = 2;
  p.weight[KSS_S_BALANCED_ALLOCATION] = 1;
  p.weight[KSS_S_IMAGE_LOCALITY] = 1;
  for (int i = 1; i <= KSS_NFILTER; i++) p.filter_enabled |= 1u << i;
  p.score_enabled = (1u << KSS_NSCORE) - 1;
  p.fit_strategy = KSS_FIT_LEAST_ALLOCATED;
  p.fit_n = 2;
  p.fit_res[0] = KSS_RES_CPU;
  p.fit_res[1] = KSS_RES_MEMORY;
  p.fit_weight[0] = 1;
  p.fit_weight[1] = 1;
  p.ba_n = 2;
  p.ba_res[0] = KSS_RES_CPU;
  p.ba_res[1] = KSS_RES_MEMORY;
  p.hard_pod_affinity_weight = 1;
  p.pct_nodes_to_score = 100;
  p.system_defaulted = 1;
  return p;
}

// Compact per-pod record of the simple path (host: build_spods): only what the
// state-dependent part of the cycle reads.  Quantities are integers held in doubles: the
// host admits a batch to this path only if every operand and every sum the loop can form
// stays below 2^53 (exact_f64 in kss_lib.hip), so all arithmetic on them is exact.
constexpr int32_t SP_ALLZERO = 1;  // computePodResourceRequest is all zero: fitsRequest checks pods only
struct SPod {
  double fit_req[3];  // NodeResourcesFit PreFilter request cpu / memory / ephemeral
  double snz[3];      // LeastAllocated request (non-zero defaults)
  double sreq[3];     // BalancedAllocation request
  double creq[3];     // AssumePod Requested delta
  double cnz[2];      // AssumePod NonZeroRequested delta
  int32_t flags;       // SP_*
  int32_t status;      // kss_pod.prefilter_status
  int32_t cls;         // class_count row the pod joins (-1 none)
  int32_t own_off, own_len;  // term_count rows it adds: ints[own_off .. +own_len) of the staged pool
  // resource shape (build_spods, kss_host.h assign_shapes): pods whose fit_req / snz / sreq / SP_ALLZERO
  // agree bit for bit share an id, numbered by first appearance; record j < (shapes of the batch)
  // also names the first pod of shape j (the shape directory the table kernel stages from)
  int32_t shape, shape_rep;
  int32_t pad;
  int64_t sc_fit[KSS_MAX_SCALAR];  // NodeResourcesFit PreFilter request of each extended (scalar) resource
  int64_t sc_req[KSS_MAX_SCALAR];  // AssumePod Requested delta of each scalar resource
};
static_assert(sizeof(SPod) % 16 == 0, "SPod is copied as uint4");
static_assert(sizeof(SPod) == 144 + 16 * KSS_MAX_SCALAR, "the shape words took SPod's padding: no growth");

// Static word of one (pod, node):
//   bits 0-2   the first failing static filter: 0 pass, 1-4 KSS_F_NODE_UNSCHEDULABLE ..
//              KSS_F_NODE_AFFINITY, 7 not evaluated (PreFilter failure, or outside the
//              NodeAffinity PreFilterResult);
//   bit 3      the pod's required node affinity matches the node (PodTopologySpread
//              NodeAffinityPolicy=Honor), bit 4 its NoSchedule/NoExecute taints are all
//              tolerated (NodeTaintsPolicy=Honor) — for every node, whatever bits 0-2 say;
//   bits 5-11  raw TaintToleration (<= 64), bits 12-31 raw NodeAffinity (host-checked:
//              Σ preferred weights < 2^20); both 0 unless bits 0-2 are 0.
constexpr uint32_t SW_NOT_EVALUATED = 7, SW_AFF_OK = 1u << 3, SW_TAINT_OK = 1u << 4;
__device__ __forceinline__ int sw_code(uint32_t w) {
  const int c = (int)(w & 7u);
  return c == (int)SW_NOT_EVALUATED ? KSS_F_NOT_EVALUATED : c;
}
__device__ __forceinline__ int sw_tt(uint32_t w) { return (int)((w >> 5) & 0x7Fu); }
__device__ __forceinline__ int sw_na(uint32_t w) { return (int)(w >> 12); }

// The ports-and-images form (PI: k_static_pi, k_simple_pi, k_simple_tab_pi) of the static word: raw
// NodeAffinity narrows to 13 bits (bits 12-24; host-checked: every pod's Σ positive preferred
// weights <= SWPI_NA_MAX) and bits 25-31 hold the ImageLocality score (0..100; final, it has no
// NormalizeScore); both 0 unless bits 0-2 are 0.  The other fields are where they were.
constexpr uint32_t SWPI_NA_BITS = 13, SWPI_NA_MAX = (1u << SWPI_NA_BITS) - 1u, SWPI_IL_SHIFT = 12 + SWPI_NA_BITS;
// A pod's NodePorts masks over the cluster's port dictionary (kss_pod.port_conflict / port_add),
// beside its SPod in the PI form: a parallel array in HBM and a ring of its own in LDS, so SPod
// does not grow.
struct alignas(16) SPort {
  uint64_t conflict, add;
};
static_assert(sizeof(SPort) == 16, "SPort is copied as uint4");

// The volumes form (VOL: k_static_vol, k_simple_vol; option simple_volumes), a variant of the PI
// form.  In a batch that only commits the volume filters never read a count: VolumeRestrictions
// reads vol_count[row][n] > 0, the limit plugins vol_count[row][n] == 0, vol_attached[key][n] and
// vol_limit[key][n], and AssumePod only ever turns a row's bit on.  So a node's volume state is one
// word of used rows (<= SV_ROWS rows) and one SV_FIELD-bit counter and limit per limit key (<=
// SV_KEYS keys, four per 64-bit word; the host checks that no field can overflow), and a pod's
// volume program is masks over the rows and counts per key: a parallel array beside SPod, like
// SPort, with a ring of its own in LDS.
constexpr int SV_KEYS = 8, SV_ROWS = 64;
constexpr uint32_t SV_UNCHECKED = 0xFFFFu;  // a limit field of vol_limit < 0 (the node does not limit the key)
constexpr uint32_t SV_FIELD_MAX = 0xFFFEu;  // the largest counter / limit a field holds
constexpr uint32_t SV_STATIC = 1u << 8;     // SVol::keys: the pod has VolumeBinding / VolumeZone entries (k_static_vol)
struct alignas(16) SVol {
  uint64_t conflict;  // rows of its KSS_VOL_CONFLICT entries
  uint64_t shared;    // rows of its KSS_VOL_LIMIT entries with row >= 0
  uint64_t own;       // rows of its KSS_VOL_OWN entries
  uint32_t keys;      // bits 0-7: keys with a KSS_VOL_LIMIT entry (checked only then); SV_STATIC; bits 16-23:
                      // keys its commit can add to (an own row of the key, or a KSS_VOL_OWN_PRIVATE count)
  uint32_t pad;
  uint16_t pnew[SV_KEYS];  // per key, the sum of `count` of its KSS_VOL_LIMIT entries with row < 0
  uint16_t padd[SV_KEYS];  // per key, its KSS_VOL_OWN_PRIVATE count
};
static_assert(sizeof(SVol) == 64, "SVol is copied as four uint4");
// One launch's constants and node-state columns of the form (a kernel argument by value).
struct SVolLaunch {
  uint64_t keyrows[SV_KEYS];  // per key, the rows counted under it (vol_row_key)
  uint32_t key_on;            // keys whose plugin the profile enables
  uint32_t key_csi;           // keys of NodeVolumeLimits (CSI: a key without a new volume is not checked)
  uint32_t vr_on;             // VolumeRestrictions enabled
  uint32_t pad;
  uint64_t* used;             // [N] rows with vol_count > 0
  uint64_t* att;              // [2][N] packed vol_attached, key k in word k / 4 at bit 16 * (k % 4)
  uint64_t* lim;              // [2][N] packed vol_limit (SV_UNCHECKED: < 0)
  const SVol* svols;          // [n_pods]
};

// lab(key): the node's interned label value (label_of by default; k_static reads an LDS copy)
template <class Lab>
__device__ __forceinline__ uint32_t static_word_l(const DevCluster& c, const DevPods& P, const kss_pod& p,
                                                  const kss_profile& prof, int n, uint32_t flags, uint64_t th,
                                                  uint64_t ts, Lab lab) {
  const int64_t g = (int64_t)c.node_base + n;
  if (p.prefilter_status != 0) return SW_NOT_EVALUATED;
  const bool aff = required_affinity_t(c, P.reqs, P.terms, P.ints, p, g, lab);
  const bool tol = (th & ~p.tol_hard) == 0;
  const uint32_t pol = (aff ? SW_AFF_OK : 0u) | (tol ? SW_TAINT_OK : 0u);
  if (p.names_len >= 0) {  // NodeAffinity PreFilterResult: nodes outside the set are not evaluated
    bool in = false;
    for (int i = 0; i < p.names_len; i++) in |= (int64_t)P.ints[p.names_off + i] == g;
    if (!in) return pol | SW_NOT_EVALUATED;
  }
  const uint32_t en = prof.filter_enabled;
  // RunFilterPlugins order (plugin_test.go:15-36): the first four filters are static
  if (((en >> KSS_F_NODE_UNSCHEDULABLE) & 1u) && (flags & KSS_NODE_UNSCHEDULABLE) && !(p.flags & KSS_POD_TOL_UNSCHEDULABLE))
    return pol | KSS_F_NODE_UNSCHEDULABLE;
  if (((en >> KSS_F_NODE_NAME) & 1u) && p.node_name != -1 && (int64_t)p.node_name != g) return pol | KSS_F_NODE_NAME;
  if (((en >> KSS_F_TAINT_TOLERATION) & 1u) && !tol) return pol | KSS_F_TAINT_TOLERATION;
  if (((en >> KSS_F_NODE_AFFINITY) & 1u) && !aff) return pol | KSS_F_NODE_AFFINITY;
  const uint32_t tt = (uint32_t)__popcll(ts & ~p.tol_soft);                         // TaintToleration.Score
  const uint32_t na = (uint32_t)na_score_t(c, P.reqs, P.terms, P.ints, p, g, lab);  // NodeAffinity.Score
  return pol | (tt << 5) | (na << 12);
}

__device__ __forceinline__ uint32_t static_word(const DevCluster& c, const DevPods& P, const kss_pod& p,
                                                const kss_profile& prof, int n, uint32_t flags, uint64_t th,
                                                uint64_t ts) {
  return static_word_l(c, P, p, prof, n, flags, th, ts, [&](int key) { return label_of(c, key, n); });
}

// k_static's form: the words of one pod on a lane's four nodes at once.  Every requirement of
// the pod is decoded once (scalar loads of the wave-uniform program) and matched against the
// four nodes' label values into a 4-bit mask, so the pod's program is walked once per lane
// instead of once per node and no loop diverges between the four nodes.  Word for word equal
// to static_word_l (req_match_t / required_affinity_t / na_score_t, kss_eval.cuh).
// lab(key, i): the label value id of node g[i] (-1 absent).
// The pod program is read through constant-address-space pointers (DevPodsK): a wave-uniform
// address there becomes a scalar load (the program never changes during a launch); through
// generic pointers every field was a per-lane flat load (k_static r6a: 557 vector loads per
// wave, waves waiting 77 % of their cycles).
#define KSS_CONST __attribute__((address_space(4)))
struct DevPodsK {
  const KSS_CONST kss_pod* pods;
  const KSS_CONST kss_req* reqs;
  const KSS_CONST kss_term* terms;
  const KSS_CONST int32_t* ints;
};
__device__ __forceinline__ DevPodsK pods_k(const DevPods& P) {
  return DevPodsK{(const KSS_CONST kss_pod*)P.pods, (const KSS_CONST kss_req*)P.reqs,
                  (const KSS_CONST kss_term*)P.terms, (const KSS_CONST int32_t*)P.ints};
}
template <class Ints, class Req, class Lab4>
__device__ __forceinline__ uint32_t req_mask4(const DevCluster& c, Ints ints, const Req& r,
                                              const int64_t (&g)[4], Lab4 lab) {
  const int op = r.op;
  if (op == KSS_OP_FALSE) return 0u;
  if (op == KSS_OP_TRUE) return 15u;
  uint32_t m = 0;
  if (op == KSS_OP_NAME_IN || op == KSS_OP_NAME_NOTIN) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool hit = r.ival >= 0 && g[i] == r.ival;
      m |= (uint32_t)(op == KSS_OP_NAME_IN ? hit : !hit) << i;
    }
    return m;
  }
  int32_t v[4];
#pragma unroll
  for (int i = 0; i < 4; i++) v[i] = lab(r.key, i);
  switch (op) {
    case KSS_OP_MASK:
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint64_t b = v[i] < 0 ? (r.mask >> 63) : (v[i] < 63 ? (r.mask >> v[i]) : 0ull);
        m |= (uint32_t)(b & 1ull) << i;
      }
      return m;
    case KSS_OP_IN:
    case KSS_OP_NOTIN: {
      uint32_t hit = 0;
      for (int j = 0; j < r.list_len; j++) {
        const int32_t x = ints[r.list_off + j];
#pragma unroll
        for (int i = 0; i < 4; i++) hit |= (uint32_t)(x == v[i]) << i;
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const bool b = ((hit >> i) & 1u) != 0;
        m |= (uint32_t)(op == KSS_OP_IN ? (v[i] >= 0 && b) : (v[i] < 0 || !b)) << i;
      }
      return m;
    }
    case KSS_OP_EXISTS:
    case KSS_OP_DNE:
#pragma unroll
      for (int i = 0; i < 4; i++) m |= (uint32_t)((v[i] >= 0) == (op == KSS_OP_EXISTS)) << i;
      return m;
    case KSS_OP_GT:
    case KSS_OP_LT:
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (v[i] < 0) continue;
        const int32_t gi = gp(c.key_base)[r.key] + v[i];
        if (!gp(c.value_is_int)[gi]) continue;
        const int64_t x = gp(c.value_int)[gi];
        m |= (uint32_t)(op == KSS_OP_GT ? x > r.ival : x < r.ival) << i;
      }
      return m;
    default:
      return 0u;
  }
}

template <class PV, class Term, class Lab4>
__device__ __forceinline__ uint32_t term_mask4(const DevCluster& c, const PV& P, const Term& t,
                                               const int64_t (&g)[4], Lab4 lab) {
  uint32_t m = 15u;
  for (int i = 0; i < t.req_len; i++) m &= req_mask4(c, P.ints, P.reqs[t.req_off + i], g, lab);
  return m;
}

// words w[i] of pod p on nodes n + min(i, cnt - 1), i < 4 (flags / th / ts: those nodes' columns)
template <class PV, class Pod, class Lab4>
__device__ __forceinline__ void static_words4(const DevCluster& c, const PV& P, const Pod& p,
                                              const kss_profile& prof, int n, int cnt, const uint32_t (&flags)[4],
                                              const uint64_t (&th)[4], const uint64_t (&ts)[4], Lab4 lab,
                                              uint32_t (&w)[4]) {
  if (p.prefilter_status != 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = SW_NOT_EVALUATED;
    return;
  }
  int64_t g[4];
#pragma unroll
  for (int i = 0; i < 4; i++) g[i] = (int64_t)c.node_base + n + min(i, cnt - 1);
  // nodeaffinity.RequiredNodeAffinity.Match: nodeSelector AND (OR over terms)
  uint32_t aff = 15u;
  for (int i = 0; i < p.sel_len; i++) aff &= req_mask4(c, P.ints, P.reqs[p.sel_off + i], g, lab);
  if (p.flags & KSS_POD_HAS_REQ_AFFINITY) {
    uint32_t any = 0;
    for (int t = 0; t < p.aff_len; t++) any |= term_mask4(c, P, P.terms[p.aff_off + t], g, lab);
    aff &= any;
  }
  uint32_t in = 15u;  // NodeAffinity PreFilterResult
  if (p.names_len >= 0) {
    in = 0;
    for (int j = 0; j < p.names_len; j++) {
      const int64_t x = (int64_t)P.ints[p.names_off + j];
#pragma unroll
      for (int i = 0; i < 4; i++) in |= (uint32_t)(x == g[i]) << i;
    }
  }
  uint32_t na[4] = {0, 0, 0, 0};  // NodeAffinity.Score
  for (int t = 0; t < p.pref_len; t++) {
    const auto& term = P.terms[p.pref_off + t];
    const uint32_t tm = term_mask4(c, P, term, g, lab);
#pragma unroll
    for (int i = 0; i < 4; i++)
      if ((tm >> i) & 1u) na[i] += (uint32_t)term.weight;
  }
  const uint32_t en = prof.filter_enabled;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const bool a = (aff >> i) & 1u;
    const bool tol = (th[i] & ~p.tol_hard) == 0;
    const uint32_t pol = (a ? SW_AFF_OK : 0u) | (tol ? SW_TAINT_OK : 0u);
    uint32_t r;
    if (!((in >> i) & 1u)) r = pol | SW_NOT_EVALUATED;
    else if (((en >> KSS_F_NODE_UNSCHEDULABLE) & 1u) && (flags[i] & KSS_NODE_UNSCHEDULABLE) && !(p.flags & KSS_POD_TOL_UNSCHEDULABLE))
      r = pol | KSS_F_NODE_UNSCHEDULABLE;
    else if (((en >> KSS_F_NODE_NAME) & 1u) && p.node_name != -1 && (int64_t)p.node_name != g[i])
      r = pol | KSS_F_NODE_NAME;
    else if (((en >> KSS_F_TAINT_TOLERATION) & 1u) && !tol)
      r = pol | KSS_F_TAINT_TOLERATION;
    else if (((en >> KSS_F_NODE_AFFINITY) & 1u) && !a)
      r = pol | KSS_F_NODE_AFFINITY;
    else
      r = pol | ((uint32_t)__popcll(ts[i] & ~p.tol_soft) << 5) | (na[i] << 12);
    w[i] = r;
  }
}

// One (pod, node) result of the compact path: filter verdict and raw scores.
struct SVal {
  int f, tt, na, fit, ba;
};

// A node row as the state-dependent filter and scores read it.
struct DynRow {
  double alloc[3], req[3], nz[2];
  double inv[3];  // RN(1 / alloc), 0 for alloc 0
  int32_t pods, allowed;
};

// v[r] of a three-element row for a runtime resource id r in [0, 3), as masks: a select
// chain would be folded back into an indexed access, which puts the row in scratch.
__device__ __forceinline__ int64_t pick3m(int r, int64_t a, int64_t b, int64_t c) {
  return (a & -(int64_t)(r == 0)) | (b & -(int64_t)(r == 1)) | (c & -(int64_t)(r == 2));
}
__device__ __forceinline__ double pick3d(int r, double a, double b, double c) {
  return __longlong_as_double(pick3m(r, __double_as_longlong(a), __double_as_longlong(b), __double_as_longlong(c)));
}

// NodeResourcesFit.Score (resourceAllocationScorer.score, useRequested=false, no scalar
// resources on this path: calculateResourceAllocatableRequest skips them at request 0).
__device__ __forceinline__ int32_t fit_fast(const kss_profile& prof, const SPod& q, const DynRow& r) {
  int32_t node_score = 0, weight_sum = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= prof.fit_n) break;
    const int res = prof.fit_res[i];
    if (res >= KSS_RES_SCALAR0) continue;
    const double A = pick3d(res, r.alloc[0], r.alloc[1], r.alloc[2]);
    if (A == 0.0) continue;
    const double base = pick3d(res, r.nz[0], r.nz[1], r.req[2]);
    const double inv = pick3d(res, r.inv[0], r.inv[1], r.inv[2]);
    const double preq = pick3d(res, q.snz[0], q.snz[1], q.snz[2]);
    const int32_t w = (int32_t)prof.fit_weight[i];
    node_score += alloc_score_d(prof.fit_strategy, base + preq, A, inv) * w;
    weight_sum += w;
  }
  if (weight_sum <= 1) return weight_sum == 0 ? 0 : node_score;
  if (weight_sum == 2) return node_score >> 1;
  return small_div(node_score, weight_sum, __builtin_amdgcn_rcpf((float)weight_sum));
}

// NodeResourcesBalancedAllocation.Score (balancedResourceScorer, useRequested=true); the
// float64 operations in the reference's order, divisions correctly rounded (div_rn).
__device__ __forceinline__ int32_t ba_fast(const kss_profile& prof, const SPod& q, const DynRow& r) {
  double fr[4] = {0.0, 0.0, 0.0, 0.0};
  bool use[4] = {false, false, false, false};
  int nf = 0;
  double total = 0.0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= prof.ba_n) break;
    const int res = prof.ba_res[i];
    if (res >= KSS_RES_SCALAR0) continue;
    const double A = pick3d(res, r.alloc[0], r.alloc[1], r.alloc[2]);
    if (A == 0.0) continue;
    const double R = pick3d(res, r.req[0], r.req[1], r.req[2]) + pick3d(res, q.sreq[0], q.sreq[1], q.sreq[2]);
    const double inv = pick3d(res, r.inv[0], r.inv[1], r.inv[2]);
    double f = div_rn_d(R, A, inv);
    if (f > 1.0) f = 1.0;
    total += f;
    fr[i] = f;
    use[i] = true;
    nf++;
  }
  double sd = 0.0;
  if (nf == 2) {
    double a = 0.0, b = 0.0;
    bool got = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (!use[i]) continue;
      if (!got) {
        a = fr[i];
        got = true;
      } else {
        b = fr[i];
      }
    }
    sd = fabs((a - b) / 2.0);
  } else if (nf > 2) {
    const double mean = total / (double)nf;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (!use[i]) continue;
      const double d = fr[i] - mean;
      const double sq = d * d;
      sum = sum + sq;
    }
    sd = sqrt(sum / (double)nf);
  }
  return (int32_t)((1.0 - sd) * 100.0);  // in [0, 100]: int32 truncation == int64(...)
}

// The state-dependent rest of one evaluation: NodeResourcesFit.Filter (fitsRequest) and
// the Fit / BalancedAllocation scores, after the static word's filters.
__device__ __forceinline__ SVal dyn_eval(const kss_profile& prof, const SPod& q, uint32_t w, const DynRow& r) {
  SVal e{sw_code(w), 0, 0, 0, 0};
  if (e.f) return e;
  if ((prof.filter_enabled >> KSS_F_NODE_RESOURCES_FIT) & 1u) {
    bool bad = (int64_t)r.pods + 1 > (int64_t)r.allowed;
    if (!(q.flags & SP_ALLZERO)) {
#pragma unroll
      for (int k = 0; k < 3; k++) bad |= q.fit_req[k] > r.alloc[k] - r.req[k];
    }
    if (bad) {
      e.f = KSS_F_NODE_RESOURCES_FIT;
      return e;
    }
  }
  e.tt = sw_tt(w);
  e.na = sw_na(w);
  e.fit = fit_fast(prof, q, r);
  e.ba = ba_fast(prof, q, r);
  return e;
}

// NormalizeScore + weights + packed selectHost key of one feasible node (the scored
// branch of schedule_pod<false>: PodTopologySpread normalises to 100 without
// constraints, InterPodAffinity keeps its raw 0).  rtt / rna: reciprocals of the maxima.
__device__ __forceinline__ long long simple_key(const kss_profile& prof, const SVal& e, bool scored, int max_tt,
                                                float rtt, int max_na, float rna, uint32_t g) {
  int64_t total = 0;
  if (scored) {
    // DefaultNormalizeScore(100, reverse=true) / (100, reverse=false); quotients <= 100
    const int32_t tt = max_tt == 0 ? 100 : 100 - small_div(100 * e.tt, max_tt, rtt);
    const int32_t na = max_na != 0 ? small_div(100 * e.na, max_na, rna) : e.na;
    const uint32_t se = prof.score_enabled;
    if ((se >> KSS_S_TAINT_TOLERATION) & 1u) total += (int64_t)tt * prof.weight[KSS_S_TAINT_TOLERATION];
    if ((se >> KSS_S_NODE_AFFINITY) & 1u) total += (int64_t)na * prof.weight[KSS_S_NODE_AFFINITY];
    if ((se >> KSS_S_NODE_RESOURCES_FIT) & 1u) total += (int64_t)e.fit * prof.weight[KSS_S_NODE_RESOURCES_FIT];
    if ((se >> KSS_S_POD_TOPOLOGY_SPREAD) & 1u) total += 100 * (int64_t)prof.weight[KSS_S_POD_TOPOLOGY_SPREAD];
    if ((se >> KSS_S_BALANCED_ALLOCATION) & 1u) total += (int64_t)e.ba * prof.weight[KSS_S_BALANCED_ALLOCATION];
  }
  return (long long)(((unsigned long long)(uint32_t)total << 32) | (0xFFFFFFFFull - g));
}

// PI form, pass B: e.fit as pass A left it in its cv column (pi_fix) -> the Fit score back in
// e.fit; returns what ImageLocality adds to the selectHost key: its raw score is its final score
// (no NormalizeScore), times its weight, in the key's total field.
template <bool DEF>
__device__ __forceinline__ long long pi_key_add(const kss_profile& prof, SVal& e, bool scored) {
  const int il = e.fit >> 8;
  e.fit &= 0xFF;
  const bool on = scored && (DEF || ((prof.score_enabled >> KSS_S_IMAGE_LOCALITY) & 1u));
  return on ? (long long)((unsigned long long)(uint32_t)(il * prof.weight[KSS_S_IMAGE_LOCALITY]) << 32) : 0ll;
}

// ---------------------------------------------------------------------------
// wave reductions on the DPP network (no LDS): xor 1, xor 2, half-row mirror, row
// mirror, then row_bcast15 / row_bcast31 carry rows 0..2 into row 3; lane 63 holds the
// result.  64-bit values move as two 32-bit halves.
// ---------------------------------------------------------------------------
template <int OP>
__device__ __forceinline__ long long op_t(long long a, long long b) {
  if (OP == OP_SUM) return a + b;
  if (OP == OP_MAX) return b > a ? b : a;
  return b < a ? b : a;
}

template <int OP>
__device__ __forceinline__ constexpr long long ident_t() {
  return OP == OP_MAX ? INT64_MIN : (OP == OP_MIN ? INT64_MAX : 0);
}

template <int OP, int CTRL, int ROWS>
__device__ __forceinline__ long long dpp_step(long long v) {
  const unsigned long long id = (unsigned long long)ident_t<OP>();
  const unsigned long long u = (unsigned long long)v;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)id, (int)(uint32_t)u, CTRL, ROWS, 0xF, false);
  const uint32_t hi =
      (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(id >> 32), (int)(uint32_t)(u >> 32), CTRL, ROWS, 0xF, false);
  return op_t<OP>(v, (long long)(((unsigned long long)hi << 32) | lo));
}

template <int OP>
__device__ __forceinline__ long long wave_red(long long v) {
  v = dpp_step<OP, 0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v = dpp_step<OP, 0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v = dpp_step<OP, 0x141, 0xF>(v);  // row_half_mirror
  v = dpp_step<OP, 0x140, 0xF>(v);  // row_mirror
  v = dpp_step<OP, 0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
  v = dpp_step<OP, 0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
  const unsigned long long u = (unsigned long long)v;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), 63);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// Six non-negative 32-bit statistics {nf0, tt0, na0, nf1, tt1, na1} reduced together
// (SUM, MAX, MAX, SUM, MAX, MAX): each DPP step issues all six moves before combining,
// so the six chains overlap instead of paying the DPP latency six times.
template <int CTRL, int ROWS>
__device__ __forceinline__ void dpp_stats_step(uint32_t (&v)[6]) {
  uint32_t t[6];
#pragma unroll
  for (int i = 0; i < 6; i++) t[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[i], CTRL, ROWS, 0xF, false);
  v[0] += t[0];
  v[1] = max(v[1], t[1]);
  v[2] = max(v[2], t[2]);
  v[3] += t[3];
  v[4] = max(v[4], t[4]);
  v[5] = max(v[5], t[5]);
}

__device__ __forceinline__ void wave_red_stats(uint32_t (&v)[6]) {
  dpp_stats_step<0xB1, 0xF>(v);
  dpp_stats_step<0x4E, 0xF>(v);
  dpp_stats_step<0x141, 0xF>(v);
  dpp_stats_step<0x140, 0xF>(v);
  dpp_stats_step<0x142, 0xA>(v);
  dpp_stats_step<0x143, 0xC>(v);
#pragma unroll
  for (int i = 0; i < 6; i++) v[i] = (uint32_t)__builtin_amdgcn_readlane((int)v[i], 63);
}

// Per-wave mode's statistics of one wave, {nf0, tt0, na0, nf1, tt1, na1}: the counts by
// ballot, the TaintToleration maxima (7-bit raw values) as one packed 16-bit pair, so three
// DPP chains instead of six.  Lane-uniform results.
typedef unsigned short kss_u16x2 __attribute__((ext_vector_type(2)));
template <int CTRL, int ROWS>
__device__ __forceinline__ void dpp_pw_step(uint32_t& tp, uint32_t& n0, uint32_t& n1) {
  const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tp, CTRL, ROWS, 0xF, false);
  const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)n0, CTRL, ROWS, 0xF, false);
  const uint32_t c = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)n1, CTRL, ROWS, 0xF, false);
  tp = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(kss_u16x2, tp),
                                                              __builtin_bit_cast(kss_u16x2, a)));
  n0 = max(n0, b);
  n1 = max(n1, c);
}
__device__ __forceinline__ void wave_red_stats_pw(uint32_t (&v)[6]) {
  const uint32_t nf0 = (uint32_t)__popcll(__ballot(v[0] != 0)), nf1 = (uint32_t)__popcll(__ballot(v[3] != 0));
  uint32_t tp = v[1] | (v[4] << 16), n0 = v[2], n1 = v[5];
  dpp_pw_step<0xB1, 0xF>(tp, n0, n1);
  dpp_pw_step<0x4E, 0xF>(tp, n0, n1);
  dpp_pw_step<0x141, 0xF>(tp, n0, n1);
  dpp_pw_step<0x140, 0xF>(tp, n0, n1);
  dpp_pw_step<0x142, 0xA>(tp, n0, n1);
  dpp_pw_step<0x143, 0xC>(tp, n0, n1);
  tp = (uint32_t)__builtin_amdgcn_readlane((int)tp, 63);
  v[0] = nf0;
  v[1] = tp & 0xFFFFu;
  v[2] = (uint32_t)__builtin_amdgcn_readlane((int)n0, 63);
  v[3] = nf1;
  v[4] = tp >> 16;
  v[5] = (uint32_t)__builtin_amdgcn_readlane((int)n1, 63);
}

// The selectHost key of a wave, reduced as 32 bits when it fits: total << kb | (2^kb - 1 -
// local node index) keeps the order of the 64-bit key (total << 32 | ~global index) whenever
// every total is below 2^(32 - kb) and 2^kb > N (key_bits: 0 when they do not), and
// 0 stays "no feasible node".  One DPP max per step instead of a 64-bit compare and select.
__device__ __forceinline__ int key_bits(const kss_profile& prof, int N) {
  const uint32_t se = prof.score_enabled;
  long long tmax = 0;  // every normalised score is at most MaxNodeScore (100)
  for (int p = 0; p < KSS_NSCORE; p++)
    if ((se >> p) & 1u) tmax += 100ll * (long long)max(prof.weight[p], 0);
  const int kb = 32 - __clz((unsigned)max(N, 1));  // 2^kb > N
  return tmax < (1ll << (32 - kb)) ? kb : 0;
}
__device__ __forceinline__ uint32_t key_compress(long long key, int kb, int node_base) {
  if (!key) return 0;
  const uint32_t m = (1u << kb) - 1u;
  const uint32_t li = (0xFFFFFFFFu - (uint32_t)(unsigned long long)key) - (uint32_t)node_base;
  return ((uint32_t)((unsigned long long)key >> 32) << kb) | (m - li);
}
__device__ __forceinline__ long long key_expand(uint32_t k, int kb, int node_base) {
  if (!k) return 0;
  const uint32_t m = (1u << kb) - 1u;
  const uint32_t li = m - (k & m);
  return (long long)(((unsigned long long)(k >> kb) << 32) | (0xFFFFFFFFull - ((uint32_t)node_base + li)));
}
// The node a selectHost key names (its low word is ~global index), relative to node_base (and to
// the shard's first node lo: a slot); -1 for key 0, "no feasible node".
__device__ __forceinline__ int key_node(long long K, int node_base, int lo = 0) {
  return K ? (int)(0xFFFFFFFFu - (uint32_t)(unsigned long long)K) - node_base - lo : -1;
}
__device__ __forceinline__ long long wave_max_key(long long key, int kb, int node_base) {
  if (!kb) return wave_red<OP_MAX>(key);
  uint32_t k = key_compress(key, kb, node_base);
#define KSS_KSTEP(CTRL, ROWS) k = max(k, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)k, CTRL, ROWS, 0xF, false))
  KSS_KSTEP(0xB1, 0xF);
  KSS_KSTEP(0x4E, 0xF);
  KSS_KSTEP(0x141, 0xF);
  KSS_KSTEP(0x140, 0xF);
  KSS_KSTEP(0x142, 0xA);
  KSS_KSTEP(0x143, 0xC);
#undef KSS_KSTEP
  k = (uint32_t)__builtin_amdgcn_readlane((int)k, 63);
  return key_expand(k, kb, node_base);
}

// LDS image of the loop head: reduction scratch (double-buffered), exchange results.
constexpr int SX_RED = 16;  // per-wave reduction row: the key and up to 15 statistics (the window's 12)
struct alignas(16) SimpleHdr {
  long long red[2][MAXWAVES][SX_RED];
  long long res[4];  // winner key of the previous pod; nf, max TT, max NA of the next pod
  long long win[12];  // window (simple_sync_win): F, TT / NA of the wholly kept segments, cut shard, part, j; d, TT, NA; E2 needed
  int cutc[2][MAXWAVES];  // window cut scan: feasible nodes of the part per wave
  int cutm[MAXWAVES][2];  // ... and the waves' maxima of the kept ones
  kss_profile prof;  // a runtime (non-default) profile: indexed by resource id, so in LDS, not scratch
  int abort;
  int pad[3];
};

// Workgroup barrier that orders LDS only.  HIP's __syncthreads() also drains every
// outstanding global load (vmcnt), which would put the prefetches on the critical path.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Workgroup reduction of K values; ONE barrier.  Parity alternates between calls, so a
// fast wave writing the next reduction never overwrites a slot a slow wave still reads.
template <int K>
__device__ __forceinline__ void block_red(SimpleHdr& H, int parity, long long (&v)[K], const int (&ops)[K]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const long long r = ops[k] == OP_SUM ? wave_red<OP_SUM>(v[k])
                                         : (ops[k] == OP_MAX ? wave_red<OP_MAX>(v[k]) : wave_red<OP_MIN>(v[k]));
    if (lane == 0) H.red[parity][wave][k] = r;
  }
  lds_barrier();
#pragma unroll
  for (int k = 0; k < K; k++) {
    long long a = H.red[parity][0][k];
    for (int w = 1; w < nw; w++) a = op_apply(ops[k], a, H.red[parity][w][k]);
    v[k] = a;
  }
}

// Cross-shard exchange, wave 0 only.  v = {key, nf0, tt0, na0, nf1, tt1, na1} of this
// shard.  Publishes 8 granules {epoch, 32-bit value}, sweeps all W shards (64 per chunk,
// every load of a chunk in flight at once), then: winner = max key; the winner's shard
// (its node index / per) contributes H1, the others H0.  Results -> H.res.
__device__ __forceinline__ bool simple_exchange(SimpleHdr& H, unsigned long long* gran, const XPeers& X, int W, int wself,
                                                unsigned epoch,
                                                int* err, const long long (&v)[7], int per, int node_base, int kb) {
  const int lane = threadIdx.x & 63;
  const unsigned long long tag = (unsigned long long)epoch << 32;
  const unsigned long long key = (unsigned long long)v[0];
  if (lane < SX_VALS) {
    uint32_t x = (uint32_t)key;
    x = lane == 1 ? (uint32_t)(key >> 32) : x;
#pragma unroll
    for (int i = 1; i < 7; i++) x = lane == i + 1 ? (uint32_t)v[i] : x;
    xpub(X, gran, ((size_t)(epoch & 1) * W + wself) * SX_VALS + lane, tag | x);
  }
  const unsigned long long* base = gran + (size_t)(epoch & 1) * W * SX_VALS;
  uint32_t got[SX_CHUNKS][SX_VALS];
  long long best = 0;
#pragma unroll
  for (int ch = 0; ch < SX_CHUNKS; ch++) {
#pragma unroll
    for (int i = 0; i < SX_VALS; i++) got[ch][i] = 0;
    if (ch * 64 >= W) continue;
    const int s = ch * 64 + lane;
    const bool valid = s < W;
    long long t0_ = 0;
    for (unsigned spins = 0;; ++spins) {
      bool ok = true;
      unsigned long long g[SX_VALS];
      // every load issued (lanes past W read shard 0's granules), no exec-mask region per load
#pragma unroll
      for (int i = 0; i < SX_VALS; i++)
        g[i] = __hip_atomic_load(base + (size_t)(valid ? s : 0) * SX_VALS + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int i = 0; i < SX_VALS; i++) {
        ok &= !valid || (g[i] >> 32) == epoch;
        got[ch][i] = valid ? (uint32_t)g[i] : 0u;
      }
      if (__all(ok)) break;
      if (spin_expired(spins, t0_)) {
        if (lane == 0) {
          H.abort = 1;
          err_raise(err, 1);
        }
        return false;
      }
      spin_pause();
    }
    const long long k = (long long)(((unsigned long long)got[ch][1] << 32) | got[ch][0]);
    best = k > best ? k : best;
  }
  best = wave_max_key(best, kb, node_base);
  // the winner's shard: the one whose row range [s * per, (s + 1) * per) holds it
  const int gl = key_node(best, node_base);
  // {nf, tt, na} of every shard's hypothesis, reduced in one interleaved DPP pass
  uint32_t u[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int ch = 0; ch < SX_CHUNKS; ch++) {
    const int s = ch * 64 + lane;
    if (s >= W) continue;
    const bool h1 = gl >= s * per && gl < s * per + per;
    u[0] += h1 ? got[ch][5] : got[ch][2];
    u[1] = max(u[1], h1 ? got[ch][6] : got[ch][3]);
    u[2] = max(u[2], h1 ? got[ch][7] : got[ch][4]);
  }
  wave_red_stats(u);
  if (lane == 0) {
    H.res[0] = best;
    H.res[1] = u[0];
    H.res[2] = u[1];
    H.res[3] = u[2];
  }
  return true;
}

// Block-reduce the six partial statistics of the next pod, exchange them with the
// current pod's shard-best key, and leave {winner key, nf, max TT, max NA} in R[] of
// every lane.  False if the launch aborted (exchange timeout).
__device__ __forceinline__ bool simple_sync(SimpleHdr& H, int& parity, long long key, long long (&st)[6], int W, int w,
                                            unsigned epoch, unsigned long long* gran, const XPeers& X, int* err, int per,
                                            int node_base, int kb,
                                            long long (&R)[4], KSS_GLOBAL unsigned long long* sp) {
  {
    uint32_t u[6];
#pragma unroll
    for (int i = 0; i < 6; i++) u[i] = (uint32_t)st[i];
    wave_red_stats(u);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) H.red[parity][wave][i] = u[i];
    }
    lds_barrier();
#pragma unroll
    for (int i = 0; i < 6; i++) st[i] = H.red[parity][0][i];
    for (int wv = 1; wv < nw; wv++) {
      st[0] += H.red[parity][wv][0];
      st[3] += H.red[parity][wv][3];
#pragma unroll
      for (int i : {1, 2, 4, 5}) st[i] = max(st[i], H.red[parity][wv][i]);
    }
  }
  parity ^= 1;
  if (sp && threadIdx.x == 0) sp[4] = wall_clock64();
  if (W == 1) {  // the winner (if any) is this shard's candidate
    const bool h1 = key != 0;
    R[0] = key;
    R[1] = h1 ? st[3] : st[0];
    R[2] = h1 ? st[4] : st[1];
    R[3] = h1 ? st[5] : st[2];
    return true;
  }
  if (threadIdx.x < 64) {
    const long long v[7] = {key, st[0], st[1], st[2], st[3], st[4], st[5]};
    simple_exchange(H, gran, X, W, w, epoch, err, v, per, node_base, kb);
  }
  lds_barrier();
  if (H.abort) return false;
#pragma unroll
  for (int i = 0; i < 4; i++) R[i] = H.res[i];
  return true;
}

// The shard's node state in LDS for the whole launch (slot s = node lo + s), the per-slot
// results of the next pod (slot `cap` of the results holds the candidate node
// re-evaluated after the previous pod's commit, H1) and the static-word ring.
struct SimpleShard {
  double* r64;    // [8][cap]: allocatable cpu/mem/eph, requested cpu/mem/eph, non-zero cpu/mem (exact integers)
  double* inv;    // [3][cap]: RN(1 / allocatable)
  int32_t* r32;   // [2][cap]: pod count, allowed pods
  uint32_t* st;   // [RING][cap]: static words of the pods in flight (ring slot = pod % RING)
  int32_t* cv;    // [5][cap + CV_EXTRA]: filter verdict, TT, NA, Fit, BA (slots cap + i: H1 values)
  SPod* ring;     // [RING]: pod records (ring slot = pod % RING)
  int64_t* sc;    // [2 nsc][cap]: allocatable, then requested, of each extended (scalar) resource
  int cap, nsc;
};

constexpr int RING = 4;                // record / static-word ring slots
constexpr int CV_EXTRA = MAXWAVES;     // H1 slots past the shard's nodes: one per wave (per-wave mode)
constexpr int PW_LANES = 63;           // per-wave mode: node slots per wave (lane 63 is the wave's H1 lane)

// The shape table of k_simple_tab (simple_schedule_tab): for every resource shape c of the batch
// and every node slot s, the packed state-dependent result of dyn_eval_def(shape c, row s).
// (KSS_MAX_SHAPES shapes at most: kss.h)
struct SShape {  // what dyn_eval_def reads of a pod
  double fit_req[3], snz[2], sreq[2];
  int32_t flags, pad;
};
static_assert(sizeof(SShape) == 64, "SShape: 64 B");
constexpr int SSHAPE_WORDS = (int)(sizeof(SShape) / 8);
constexpr uint32_t ST_FITS = 1u << 16;  // table word: NodeResourcesFit passes, Fit score << 8, BalancedAllocation score
// a table row holds cap slots at a stride of cap + 1 words: the lanes that copy a pending row into
// one slot's column (lane = shape) then fall into different LDS banks
__host__ __device__ inline size_t shape_tab_bytes(int cap, int n_shapes) {
  return n_shapes > 0 ? (size_t)n_shapes * sizeof(SShape) + 4 * (size_t)MAXWAVES * KSS_MAX_SHAPES +
                            4 * (size_t)n_shapes * ((size_t)cap + 1)
                      : 0;
}
// rounds of one refresh: candidates x shapes evaluations on the lanes of every wave but wave 0
__host__ __device__ inline int shape_tab_rounds(int nwave, int n_shapes) {
  const int idle = 64 * (nwave - 1);
  return idle > 0 ? (nwave * n_shapes + idle - 1) / idle : 0;
}

__host__ __device__ inline size_t simple_lds_bytes(int cap, int nsc = 0, int n_shapes = 0) {
  const size_t base = sizeof(SimpleHdr) + RING * sizeof(SPod) +
                      (size_t)cap * (8 * 8 + 3 * 8 + 2 * 4 + RING * 4 + 16 * (size_t)nsc) + 20 * ((size_t)cap + CV_EXTRA);
  return n_shapes > 0 ? (base + 15) / 16 * 16 + shape_tab_bytes(cap, n_shapes) : base;
}

// The PI form's LDS behind the shard's (no shape table in this form): the ring of the pods' port
// masks (ring slot = pod % RING, as the record ring) and the UsedPorts column, one word per slot.
__host__ __device__ inline size_t simple_lds_bytes_pi(int cap, int nsc) {
  return (simple_lds_bytes(cap, nsc) + 15) / 16 * 16 + RING * sizeof(SPort) + 8 * (size_t)cap;
}

// The volumes form's LDS behind the PI form's: the used-rows column, the packed attached / limit
// columns (two words each), the keys' row masks, and the ring of the pods' SVol records.
__host__ __device__ inline size_t simple_lds_bytes_vol(int cap, int nsc) {
  return (simple_lds_bytes_pi(cap, nsc) + 15) / 16 * 16 + 40 * (size_t)cap + 8 * SV_KEYS + RING * sizeof(SVol);
}

struct ShapeTab {
  uint64_t* shp;   // [SSHAPE_WORDS][n_shapes]: the shapes' SShape records, staged once per launch, word by word
                   // (lane = shape reads consecutive words: no bank conflict)
  uint32_t* pnd;   // [MAXWAVES][KSS_MAX_SHAPES]: wave v's candidate with the pod committed, per shape
  uint32_t* T;     // [n_shapes][ts]
  int n, ts;       // shapes, row stride (cap + 1)
};
__device__ __forceinline__ SShape shape_get(const ShapeTab& t, int j) {
  uint64_t w[SSHAPE_WORDS];
#pragma unroll
  for (int i = 0; i < SSHAPE_WORDS; i++) w[i] = t.shp[i * t.n + j];
  SShape q;
  __builtin_memcpy(&q, w, sizeof(SShape));
  return q;
}
__device__ __forceinline__ ShapeTab shape_tab_view(uint8_t* smem0, int cap, int n_shapes) {
  uint8_t* b = smem0 + (simple_lds_bytes(cap, 0) + 15) / 16 * 16;
  ShapeTab t;
  t.n = n_shapes;
  t.ts = cap + 1;
  t.shp = reinterpret_cast<uint64_t*>(b);
  t.pnd = reinterpret_cast<uint32_t*>(b + (size_t)n_shapes * sizeof(SShape));
  t.T = t.pnd + MAXWAVES * KSS_MAX_SHAPES;
  return t;
}
__device__ __forceinline__ uint32_t shape_pack(const SVal& e) {
  return (e.f == 0 ? ST_FITS : 0u) | (((uint32_t)e.fit & 0xFFu) << 8) | ((uint32_t)e.ba & 0xFFu);
}

__device__ __forceinline__ SimpleShard shard_view(uint8_t* base, int cap, int nsc) {
  SimpleShard L;
  L.cap = cap;
  L.nsc = nsc;
  L.ring = reinterpret_cast<SPod*>(base);
  L.sc = reinterpret_cast<int64_t*>(base + RING * sizeof(SPod));
  uint8_t* b = base + RING * sizeof(SPod) + 16 * (size_t)nsc * (size_t)cap;
  L.r64 = reinterpret_cast<double*>(b);
  L.inv = reinterpret_cast<double*>(b + 64 * (size_t)cap);
  L.r32 = reinterpret_cast<int32_t*>(b + 88 * (size_t)cap);
  L.st = reinterpret_cast<uint32_t*>(L.r32 + 2 * (size_t)cap);
  L.cv = reinterpret_cast<int32_t*>(L.st + RING * (size_t)cap);
  return L;
}

__device__ __forceinline__ DynRow shard_row(const SimpleShard& L, int s) {
  DynRow r;
  const int C = L.cap;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    r.alloc[k] = L.r64[k * C + s];
    r.req[k] = L.r64[(3 + k) * C + s];
    r.inv[k] = L.inv[k * C + s];
  }
  r.nz[0] = L.r64[6 * C + s];
  r.nz[1] = L.r64[7 * C + s];
  r.pods = L.r32[s];
  r.allowed = L.r32[C + s];
  return r;
}

__device__ __forceinline__ SVal cv_get(const SimpleShard& L, int s) {
  const int C1 = L.cap + CV_EXTRA;
  return SVal{L.cv[s], L.cv[C1 + s], L.cv[2 * C1 + s], L.cv[3 * C1 + s], L.cv[4 * C1 + s]};
}

__device__ __forceinline__ void cv_put(const SimpleShard& L, int s, const SVal& e) {
  const int C1 = L.cap + CV_EXTRA;
  L.cv[s] = e.f;
  L.cv[C1 + s] = e.tt;
  L.cv[2 * C1 + s] = e.na;
  L.cv[3 * C1 + s] = e.fit;
  L.cv[4 * C1 + s] = e.ba;
}

// NodeResourcesFit.Filter over the extended (scalar) resources (fitsRequest; a zero request
// is skipped): true when some requested scalar exceeds the node's free amount.  sc: [2 nsc][cap]
// allocatable, then requested; add: pod q0's AssumePod delta is added to the row first (H1).
__device__ __forceinline__ bool scalar_short(const int64_t* sc, int nsc, int cap, int s, const SPod& q, bool add,
                                             const SPod& q0) {
  bool bad = false;
#pragma unroll
  for (int i = 0; i < KSS_MAX_SCALAR; i++) {
    if (i >= nsc) break;
    const int64_t req = q.sc_fit[i];
    const int64_t used = sc[(size_t)(nsc + i) * cap + s] + (add ? q0.sc_req[i] : 0);
    bad |= req != 0 && req > sc[(size_t)i * cap + s] - used;
  }
  return bad;
}

// NodeInfo.AddPod on a node row (requested, non-zero requested, pod count).
__device__ __forceinline__ void add_commit(DynRow& r, const SPod& p) {
#pragma unroll
  for (int k = 0; k < 3; k++) r.req[k] += p.creq[k];
  r.nz[0] += p.cnz[0];
  r.nz[1] += p.cnz[1];
  r.pods += 1;
}

// leastRequestedScore for the branch-free default-profile evaluation: 0 when requested >
// capacity; the caller masks capacity 0 (inv 0).
__device__ __forceinline__ int32_t least_bf(double requested, double capacity, double inv) {
  const bool over = requested > capacity;
  const double x = (capacity - (over ? capacity : requested)) * 100.0;  // integers below 2^53: exact, >= 0
  int32_t q = (int32_t)(x * inv);
  const double r = fma(-(double)q, capacity, x);
  q += (r >= capacity ? 1 : 0) - (r < 0.0 ? 1 : 0);
  return over ? 0 : q;
}

// dyn_eval of the v1.26 default profile (NodeResourcesFit LeastAllocated over cpu / memory
// with weights 1 / 1, BalancedAllocation over cpu / memory), branch-free: every lane
// computes every score and selects, so the node loop carries no exec-mask regions.  The
// scores of an infeasible node are not read (pass B skips it).
// Q: SPod, or the resource shape alone (SShape: the same fields under the same names).
template <class Q>
__device__ __forceinline__ SVal dyn_eval_def(const Q& q, uint32_t w, const DynRow& r) {
  const int code = sw_code(w);
  bool bad = (int64_t)r.pods + 1 > (int64_t)r.allowed;
  const bool rq = !(q.flags & SP_ALLZERO);
  bad |= rq & ((q.fit_req[0] > r.alloc[0] - r.req[0]) | (q.fit_req[1] > r.alloc[1] - r.req[1]) |
               (q.fit_req[2] > r.alloc[2] - r.req[2]));
  SVal e;
  e.f = code ? code : (bad ? KSS_F_NODE_RESOURCES_FIT : 0);
  e.tt = sw_tt(w);
  e.na = sw_na(w);
  const bool u0 = r.alloc[0] != 0.0, u1 = r.alloc[1] != 0.0;
  // NodeResourcesFit.Score: capacity-0 resources drop out of the score and the weight sum
  const int32_t s0 = u0 ? least_bf(r.nz[0] + q.snz[0], r.alloc[0], r.inv[0]) : 0;
  const int32_t s1 = u1 ? least_bf(r.nz[1] + q.snz[1], r.alloc[1], r.inv[1]) : 0;
  e.fit = (u0 && u1) ? (s0 + s1) >> 1 : s0 + s1;
  // BalancedAllocation: two used resources give |f0 - f1| / 2, fewer a zero deviation
  double f0 = div_rn_d(r.req[0] + q.sreq[0], r.alloc[0], r.inv[0]);
  double f1 = div_rn_d(r.req[1] + q.sreq[1], r.alloc[1], r.inv[1]);
  f0 = f0 > 1.0 ? 1.0 : f0;
  f1 = f1 > 1.0 ? 1.0 : f1;
  const double sd = (u0 && u1) ? fabs((f0 - f1) / 2.0) : 0.0;
  e.ba = (int32_t)((1.0 - sd) * 100.0);
  return e;
}

// PI form, after an evaluation on a PI static word (whose e.na still carries the ImageLocality
// score above the 13 NodeAffinity bits): the NodePorts verdict (used: the node's UsedPorts bits,
// with the previous pod's port_add in the H1 evaluation; a node failing NodeResourcesFit keeps
// that verdict -- an unrecorded batch shows only that the node is infeasible), the NodeAffinity
// field, and the ImageLocality score moved above the Fit score (<= 100), the cv column in which it
// reaches pass B.
template <bool DEF>
__device__ __forceinline__ void pi_fix(const kss_profile& prof, SVal& e, uint64_t used, uint64_t conflict) {
  const bool en = DEF || ((prof.filter_enabled >> KSS_F_NODE_PORTS) & 1u);
  e.f = (e.f == 0 && en && (used & conflict) != 0) ? KSS_F_NODE_PORTS : e.f;
  const int il = e.na >> SWPI_NA_BITS;
  e.na &= (int)SWPI_NA_MAX;
  e.fit |= il << 8;
}

// The volumes form's LDS (simple_lds_bytes_vol) and launch constants as pass A and the commit see them.
struct VolView {
  uint64_t* used;         // [cap]
  uint64_t* att;          // [2][cap]
  uint64_t* lim;          // [2][cap]
  const uint64_t* keyrows;  // [SV_KEYS]
  SVol* ring;             // [RING]
  uint32_t key_on, key_csi, vr_on;
  int cap;
};
__device__ __forceinline__ VolView vol_view(uint8_t* smem0, int cap, int nsc, const SVolLaunch& K) {
  uint8_t* b = smem0 + (simple_lds_bytes_pi(cap, nsc) + 15) / 16 * 16;
  VolView V;
  V.cap = cap;
  V.used = reinterpret_cast<uint64_t*>(b);
  V.att = V.used + cap;
  V.lim = V.att + 2 * (size_t)cap;
  uint64_t* kr = V.lim + 2 * (size_t)cap;
  V.keyrows = kr;
  V.ring = reinterpret_cast<SVol*>(kr + SV_KEYS);
  V.key_on = K.key_on;
  V.key_csi = K.key_csi;
  V.vr_on = K.vr_on;
  return V;
}

// AssumePod of pod p's volumes on a node's state in registers (vol_commit_row over its KSS_VOL_OWN
// rows, then its KSS_VOL_OWN_PRIVATE counts): a row not yet used adds one to its key's counter,
// then the row is used.  The key mask is wave-uniform: a scalar loop over its set bits.
__device__ __forceinline__ void vol_assume(const VolView& V, const SVol& p, uint64_t& used, uint64_t& a0, uint64_t& a1) {
  const uint64_t own = p.own;
  for (uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)((p.keys >> 16) & 0xFFu)); m; m &= m - 1) {
    const int k = __builtin_ctz(m), sh = (k & 3) * 16;
    const uint64_t d = (uint64_t)(__builtin_popcountll(own & ~used & V.keyrows[k]) + (int)p.padd[k]) << sh;
    if (k < 4) a0 += d;
    else a1 += d;
  }
  used |= own;
}

// The dynamic volume filters of pod q (ring slot vq) on slot ns: VolumeRestrictions (a row of its
// conflict mask is used) and the attach-limit plugins, limit_exceeded (kss_eval.cuh) restated on the
// packed fields for every key of the pod's key mask.  extra: the H1 evaluation, on the state after
// pod p's (ring slot vp) AssumePod.
__device__ __forceinline__ bool vol_infeasible(const VolView& V, int ns, bool extra, int vq, int vp) {
  const SVol& q = V.ring[vq];
  uint64_t used = V.used[ns], a0 = V.att[ns], a1 = V.att[V.cap + ns];
  const uint64_t l0 = V.lim[ns], l1 = V.lim[V.cap + ns];
  if (extra) vol_assume(V, V.ring[vp], used, a0, a1);
  bool bad = V.vr_on && (used & q.conflict) != 0;
  const uint64_t fresh = q.shared & ~used;
  for (uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)(q.keys & 0xFFu & V.key_on)); m; m &= m - 1) {
    const int k = __builtin_ctz(m), sh = (k & 3) * 16;
    const uint32_t a = (uint32_t)((k < 4 ? a0 : a1) >> sh) & 0xFFFFu, l = (uint32_t)((k < 4 ? l0 : l1) >> sh) & 0xFFFFu;
    const uint32_t nw = (uint32_t)__builtin_popcountll(fresh & V.keyrows[k]) + q.pnew[k];
    const bool csi = (V.key_csi >> k) & 1u;
    bad |= l != SV_UNCHECKED && !(csi && nw == 0) && a + nw > l;
  }
  return bad;
}

// ... and pod p's AssumePod on slot s of the columns (simple_commit_lanes, one lane)
__device__ __forceinline__ void vol_commit(const VolView& V, int s, int vp) {
  uint64_t used = V.used[s], a0 = V.att[s], a1 = V.att[V.cap + s];
  vol_assume(V, V.ring[vp], used, a0, a1);
  V.used[s] = used;
  V.att[s] = a0;
  V.att[V.cap + s] = a1;
}

// Pass A for pod q (static words in ring slot `sl`) over the shard's `own` nodes on the
// current state (H0), plus the candidate slot `cand_s` (-1 none) re-evaluated with the
// previous pod `q0` committed on it (H1), by the first slot without a node (slot `own`,
// which is slot `cap` of lane 0 when the shard is full).  st = {nf0, tt0, na0, nf1, tt1, na1}.
// Both records are copied to registers before the node loop (its LDS stores would otherwise
// make the compiler re-read every record field inside the loop, one LDS round trip each).
// VOL (all four pass-A functions): the volumes form; a node that passed so far fails on pod q's
// dynamic volume filters (vol_infeasible; V: the columns, vq / vp: the ring slots of q's and q0's SVol).
template <bool DEF, bool PI = false, bool VOL = false>
__device__ __forceinline__ void simple_pass_a(const kss_profile& prof, const SPod& q_lds, const SPod& q0_lds,
                                              const SimpleShard& L, int sl, int own, int cand_s, long long (&st)[6],
                                              const uint64_t* pused = nullptr, SPort qp = SPort{}, uint64_t q0add = 0,
                                              const VolView* V = nullptr, int vq = 0, int vp = 0) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const uint32_t* sw = L.st + (size_t)sl * L.cap;
  const SPod q = q_lds;
  SPod q0;
#pragma unroll
  for (int k = 0; k < 3; k++) q0.creq[k] = q0_lds.creq[k];
  q0.cnz[0] = q0_lds.cnz[0];
  q0.cnz[1] = q0_lds.cnz[1];
  // extended resources: read from the LDS records inside the (rare) branch, not copied here
  const bool scal = L.nsc > 0 && (DEF || ((prof.filter_enabled >> KSS_F_NODE_RESOURCES_FIT) & 1u));
  int32_t nf = 0, tt = 0, na = 0, nf1 = 0, tt1 = 0, na1 = 0;  // raw TT <= 64, NA < 2^20
  for (int s = tid; s <= L.cap; s += nt) {
    const bool extra = s == own && cand_s >= 0;
    if (s >= own && !extra) continue;
    const int ns = extra ? cand_s : s;
    const uint32_t wd = sw[ns];
    DynRow r = shard_row(L, ns);
    if (extra) add_commit(r, q0);
    SVal e = DEF ? dyn_eval_def(q, wd, r) : dyn_eval(prof, q, wd, r);
    if constexpr (PI) pi_fix<DEF>(prof, e, pused[ns] | (extra ? q0add : 0ull), qp.conflict);
    if constexpr (VOL) e.f = (e.f == 0 && vol_infeasible(*V, ns, extra, vq, vp)) ? KSS_F_VOLUME_RESTRICTIONS : e.f;
    if (scal && e.f == 0 && scalar_short(L.sc, L.nsc, L.cap, ns, q_lds, extra, q0_lds)) e.f = KSS_F_NODE_RESOURCES_FIT;
    cv_put(L, extra ? L.cap : s, e);
    // H0 counts the shard's own slots, H1 every slot but the candidate's (whose H1 value is
    // the extra slot's); selects, no exec-mask region
    const bool c0 = e.f == 0 && !extra, c1 = e.f == 0 && s != cand_s;
    nf += c0 ? 1 : 0;
    tt = max(tt, c0 ? e.tt : 0);
    na = max(na, c0 ? e.na : 0);
    nf1 += c1 ? 1 : 0;
    tt1 = max(tt1, c1 ? e.tt : 0);
    na1 = max(na1, c1 ? e.na : 0);
  }
  st[0] = nf;
  st[1] = tt;
  st[2] = na;
  st[3] = nf1;
  st[4] = tt1;
  st[5] = na1;
}

// Per-wave mode (every shard's nodes fit in PW_LANES slots per wave, one per lane): wave v
// owns slots [v * pwv, v * pwv + pwv) of its shard and its lane pwv re-evaluates the WAVE's best
// candidate of the previous pod with that pod committed (the wave's H1).  The shard then never
// reduces its best key by itself: the waves' bests ride with the statistics, one workgroup
// reduction per pod instead of two (simple_sync_pw).  u = the wave lane's {nf0, tt0, na0, nf1,
// tt1, na1} (H1: the wave's slots but its candidate, plus the candidate re-evaluated).
template <bool DEF, bool PI = false, bool VOL = false>
__device__ __forceinline__ void simple_pass_a_pw(const kss_profile& prof, const SPod& q_lds, const SPod& q0_lds,
                                                 const SimpleShard& L, int sl, int own, int pwv, int cand_w,
                                                 uint32_t (&u)[6], const uint64_t* pused = nullptr, SPort qp = SPort{},
                                                 uint64_t q0add = 0, const VolView* V = nullptr, int vq = 0, int vp = 0) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t* sw = L.st + (size_t)sl * L.cap;
  const SPod q = q_lds;
  SPod q0;
#pragma unroll
  for (int k = 0; k < 3; k++) q0.creq[k] = q0_lds.creq[k];
  q0.cnz[0] = q0_lds.cnz[0];
  q0.cnz[1] = q0_lds.cnz[1];
  // extended resources: read from the LDS records inside the (rare) branch, not copied here
  const bool scal = L.nsc > 0 && (DEF || ((prof.filter_enabled >> KSS_F_NODE_RESOURCES_FIT) & 1u));
  const int s = wv * pwv + lane;
  const bool extra = lane == pwv && cand_w >= 0;
  const bool mine = lane < pwv && s < own;
#pragma unroll
  for (int i = 0; i < 6; i++) u[i] = 0;
  if (mine || extra) {
    const int ns = extra ? cand_w : s;
    const uint32_t wd = sw[ns];
    DynRow r = shard_row(L, ns);
    if (extra) add_commit(r, q0);
    SVal e = DEF ? dyn_eval_def(q, wd, r) : dyn_eval(prof, q, wd, r);
    if constexpr (PI) pi_fix<DEF>(prof, e, pused[ns] | (extra ? q0add : 0ull), qp.conflict);
    if constexpr (VOL) e.f = (e.f == 0 && vol_infeasible(*V, ns, extra, vq, vp)) ? KSS_F_VOLUME_RESTRICTIONS : e.f;
    if (scal && e.f == 0 && scalar_short(L.sc, L.nsc, L.cap, ns, q_lds, extra, q0_lds)) e.f = KSS_F_NODE_RESOURCES_FIT;
    cv_put(L, extra ? L.cap + wv : s, e);
    const bool c0 = e.f == 0 && !extra, c1 = e.f == 0 && (extra || s != cand_w);
    u[0] = c0 ? 1u : 0u;
    u[1] = c0 ? (uint32_t)e.tt : 0u;
    u[2] = c0 ? (uint32_t)e.na : 0u;
    u[3] = c1 ? 1u : 0u;
    u[4] = c1 ? (uint32_t)e.tt : 0u;
    u[5] = c1 ? (uint32_t)e.na : 0u;
  }
}

// AssumePod of pk on shard slot s (LDS node rows; the class / term counts follow after the
// launch, k_counts), spread over the lanes of one wave: lane r < 5 adds row 3 + r (Requested cpu /
// memory / ephemeral, then NonZeroRequested cpu / memory: creq and cnz are adjacent), lane 5 the
// pod count, lanes 8.. the extended resources -- the rows' LDS round trips overlap instead of
// following each other on one lane (r7c A/B against one lane adding every row: C2 284.7k ->
// 290.7k pods/s, C4 unchanged; the one-lane form is retired, DESIGN.md "Retired A/B switches").
static_assert(offsetof(SPod, cnz) == offsetof(SPod, creq) + 3 * sizeof(double), "creq, cnz adjacent");
template <bool PI = false, bool VOL = false>
__device__ __forceinline__ void simple_commit_lanes(const SimpleShard& L, const SPod& pk, int s, int lane,
                                                    uint64_t* pused = nullptr, uint64_t padd = 0,
                                                    const VolView* V = nullptr, int vp = 0) {
  const int cap = L.cap;
  if constexpr (PI) {  // NodeInfo.UsedPorts: the pod's host ports
    if (lane == 6) pused[s] |= padd;
  }
  if constexpr (VOL) {  // the pod's volumes, on the free lane next to it
    if (lane == 7) vol_commit(*V, s, vp);
  }
  if (lane < 5) L.r64[(3 + lane) * cap + s] += (&pk.creq[0])[lane];
  if (lane == 5) L.r32[s] += 1;
  if (lane >= 8 && lane < 8 + L.nsc) L.sc[(size_t)(L.nsc + lane - 8) * cap + s] += pk.sc_req[lane - 8];
}

// Per-wave mode's one reduction per pod: the waves' best keys and H0 / H1 statistics in one
// LDS pass (the shard's H1 is the best wave's H1 with every other wave's H0), the cross-shard
// exchange, and pod k's AssumePod on the winner's slot by wave 0 BEFORE the closing barrier
// (the next pod's pass A reads that row with no barrier of its own in between).
// R = {winner key, nf, max TT, max NA of the next pod}.  False if the launch aborted.
// `idle` runs on every wave right after the statistics barrier: the waves other than wave 0
// wait out the exchange there (the prefetch loads are issued from it).
// Wave 0 alone polls the exchange and a closing barrier hands the result to the others.  Every
// wave polling for itself, with no closing barrier, lost (r8t A/B: C2 261k against 304k pods/s):
// the prefetch waves' polls queue behind their own HBM prefetch loads (vmcnt is in order), so
// the pod waits for them.  (Retired: DESIGN.md "Retired A/B switches".)
template <bool PI = false, bool VOL = false, typename Idle>
__device__ __forceinline__ bool simple_sync_pw(SimpleHdr& H, int& parity, long long wbest, uint32_t (&u)[6], int W,
                                               int w, unsigned epoch, unsigned long long* gran, const XPeers& X,
                                               int* err, int per, int node_base, int lo, int own, const SPod& pk,
                                               bool commit, const SimpleShard& L, int kb, long long (&R)[4],
                                               KSS_GLOBAL unsigned long long* sp, Idle&& idle,
                                               uint64_t* pused = nullptr, uint64_t padd = 0, const VolView* V = nullptr, int vp = 0) {
  wave_red_stats_pw(u);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (sp && threadIdx.x == 0) sp[7] = wall_clock64();
  if (sp && (threadIdx.x == 64 || threadIdx.x == 128)) sp[9 + (threadIdx.x >> 6)] = wall_clock64();  // waves 1, 2 reach it
  if (lane == 0) {
    H.red[parity][wave][0] = wbest;
#pragma unroll
    for (int i = 0; i < 6; i++) H.red[parity][wave][1 + i] = u[i];
  }
  lds_barrier();
  if (sp && threadIdx.x == 0) sp[8] = wall_clock64();
  idle();
  if (wave == 0) {  // wave 0 alone combines (every lane the same few LDS words: broadcasts) and exchanges
    // lane v < nw reads wave v's partials (one LDS round trip for all waves), then three DPP
    // steps over the (at most 8) lanes: the largest key, and the six statistics with the best
    // wave contributing its H1 (r7d A/B against every lane reading the waves' rows in turn: C2
    // 291.8k -> 301.3k pods/s)
    const bool in = lane < nw;
    const long long* hv = H.red[parity][in ? lane : 0];
    const long long kv = in ? hv[0] : 0;
    uint32_t xv[6];
#pragma unroll
    for (int i = 0; i < 6; i++) xv[i] = in ? (uint32_t)hv[1 + i] : 0u;
    long long best = kv;
    best = dpp_step<OP_MAX, 0xB1, 0xF>(best);
    best = dpp_step<OP_MAX, 0x4E, 0xF>(best);
    best = dpp_step<OP_MAX, 0x141, 0xF>(best);
    {
      const unsigned long long ub = (unsigned long long)best;
      best = (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(ub >> 32), 0) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ub, 0));
    }
    const bool me = in && best != 0 && kv == best;  // keys carry the node index: one wave at most
    uint32_t t[6] = {xv[0], xv[1], xv[2], me ? xv[3] : xv[0], me ? xv[4] : xv[1], me ? xv[5] : xv[2]};
    dpp_stats_step<0xB1, 0xF>(t);
    dpp_stats_step<0x4E, 0xF>(t);
    dpp_stats_step<0x141, 0xF>(t);
#pragma unroll
    for (int i = 0; i < 6; i++) t[i] = (uint32_t)__builtin_amdgcn_readlane((int)t[i], 0);
    if (sp && lane == 0) sp[4] = wall_clock64();
    if (W == 1) {  // the winner (if any) is this shard's best
      const bool h1 = best != 0;
      const int slot = (int)(0xFFFFFFFFu - (uint32_t)(unsigned long long)best) - node_base - lo;
      if (lane == 0) {
        H.res[0] = best;
        H.res[1] = h1 ? t[3] : t[0];
        H.res[2] = h1 ? t[4] : t[1];
        H.res[3] = h1 ? t[5] : t[2];
      }
      if (commit && h1) simple_commit_lanes<PI, VOL>(L, pk, slot, lane, pused, padd, V, vp);
    } else {
      const long long v[7] = {best, t[0], t[1], t[2], t[3], t[4], t[5]};
      if (simple_exchange(H, gran, X, W, w, epoch, err, v, per, node_base, kb) && commit) {
        const long long K = H.res[0];  // (written by lane 0 of this wave: in order)
        const int x = key_node(K, node_base, lo);
        if (x >= 0 && x < own) simple_commit_lanes<PI, VOL>(L, pk, x, lane, pused, padd, V, vp);
      }
    }
  }
  parity ^= 1;
  lds_barrier();
  if (H.abort) return false;
#pragma unroll
  for (int i = 0; i < 4; i++) R[i] = H.res[i];
  return true;
}

// ---------------------------------------------------------------------------
// percentageOfNodesToScore < 100: findNodesThatPassFilters' window on k_simple
// ---------------------------------------------------------------------------
// v1.26 findNodesThatPassFilters (Parallelism = 1, the deterministic form) checks
// the nodes from nextStartNodeIndex s in canonical order, wrapping, and stops once K + 1 feasible
// nodes were found (K = numFeasibleNodesToFind): the first K are kept (scored, selectHost's
// candidates); the (K+1)-th, d, was filtered but dropped, and nextStartNodeIndex becomes d (the
// processed count is the d - s nodes before it).  With F <= K feasible nodes every node is
// visited, every feasible one kept, and s stays.
// Here the window rides on the pod's statistics exchange.  Each shard splits its slots at the
// pod's start node into part a (node >= s) and part b (node < s), so the visiting order is the
// segments a_0 .. a_{W-1}, b_0 .. b_{W-1}, and publishes per part {feasible count, max raw TT,
// max raw NA} for H0 and H1 (SXW_VALS granules).  After the sweep every shard knows from the
// segments' counts the segment holding the (K+1)-th feasible node (the cut) and the maxima of
// the segments wholly before it.  Only the cut segment's shard needs d: every other shard's
// segments lie wholly before or after the cut, so pass B keeps node n iff feasible and (no cut,
// or seg(n) < cut segment, or seg(n) == cut segment and n < d), and the next pod's split needs
// only the start SHARD elsewhere (shards before it: every node in part b; after it: part a).
// The cut shard ranks its feasible nodes (ballots) for d and the maxima over its first j; a
// second exchange (SXW_E2 granules, polled from that one shard) carries those maxima only when
// the cut segment's maxima over ALL its feasible nodes exceed the wholly kept segments' (known
// to every shard from the first exchange): otherwise they cannot change the result.
// Statistics index: (h * 2 + part) * 3 + {0 F, 1 TT, 2 NA}, h = 0 H0, 1 H1.
constexpr int SXW_VALS = 10;  // granules per shard: key lo / hi, then {F << 16 | TT, NA} of a0, b0, a1, b1
constexpr int SXW_E2 = 4;     // the cut shard's granules per epoch parity: d, TT, NA (+ pad)
constexpr int SXW_CUR = 2;    // split grids: the end-of-launch cursor granule behind the cut granules (+ pad)
// The window's granules of one launch (8-byte words of the exchange buffer / an inbox half).
constexpr size_t sxw_words(int W) { return 2 * (size_t)W * SXW_VALS + 2 * SXW_E2 + SXW_CUR; }
// Where an XCD-local grid's claim counters sit in the exchange buffer of k_simple and its forms
// (claim_xcd_shard's ctr_off): behind the statistics granules, under the window behind its cut granules.
template <bool WIN>
__host__ __device__ constexpr size_t xcd_ctr_off(int W) {
  return WIN ? 2 * (size_t)W * SXW_VALS + 2 * SXW_E2 : 2 * (size_t)W * SX_VALS;
}

__device__ __forceinline__ void win_acc(uint32_t (&u)[12], bool c0, bool c1, int part, const SVal& e) {
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const bool on = ((v >> 1) ? c1 : c0) && (v & 1) == part;
    u[v * 3] += on ? 1u : 0u;
    u[v * 3 + 1] = max(u[v * 3 + 1], on ? (uint32_t)e.tt : 0u);
    u[v * 3 + 2] = max(u[v * 3 + 2], on ? (uint32_t)e.na : 0u);
  }
}

// simple_pass_a with the window's split: part a / b of each slot by its node against `start`
template <bool DEF, bool PI = false, bool VOL = false>
__device__ __forceinline__ void simple_pass_a_win(const kss_profile& prof, const SPod& q_lds, const SPod& q0_lds,
                                                  const SimpleShard& L, int sl, int own, int cand_s, int lo, int start,
                                                  uint32_t (&u)[12], const uint64_t* pused = nullptr, SPort qp = SPort{},
                                                  uint64_t q0add = 0, const VolView* V = nullptr, int vq = 0, int vp = 0) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const uint32_t* sw = L.st + (size_t)sl * L.cap;
  const SPod q = q_lds;
  SPod q0;
#pragma unroll
  for (int k = 0; k < 3; k++) q0.creq[k] = q0_lds.creq[k];
  q0.cnz[0] = q0_lds.cnz[0];
  q0.cnz[1] = q0_lds.cnz[1];
  const bool scal = L.nsc > 0 && (DEF || ((prof.filter_enabled >> KSS_F_NODE_RESOURCES_FIT) & 1u));
#pragma unroll
  for (int i = 0; i < 12; i++) u[i] = 0;
  for (int s = tid; s <= L.cap; s += nt) {
    const bool extra = s == own && cand_s >= 0;
    if (s >= own && !extra) continue;
    const int ns = extra ? cand_s : s;
    const uint32_t wd = sw[ns];
    DynRow r = shard_row(L, ns);
    if (extra) add_commit(r, q0);
    SVal e = DEF ? dyn_eval_def(q, wd, r) : dyn_eval(prof, q, wd, r);
    if constexpr (PI) pi_fix<DEF>(prof, e, pused[ns] | (extra ? q0add : 0ull), qp.conflict);
    if constexpr (VOL) e.f = (e.f == 0 && vol_infeasible(*V, ns, extra, vq, vp)) ? KSS_F_VOLUME_RESTRICTIONS : e.f;
    if (scal && e.f == 0 && scalar_short(L.sc, L.nsc, L.cap, ns, q_lds, extra, q0_lds)) e.f = KSS_F_NODE_RESOURCES_FIT;
    cv_put(L, extra ? L.cap : s, e);
    win_acc(u, e.f == 0 && !extra, e.f == 0 && s != cand_s, lo + ns >= start ? 0 : 1, e);
  }
}

// simple_pass_a_pw with the window's split
template <bool DEF, bool PI = false, bool VOL = false>
__device__ __forceinline__ void simple_pass_a_pw_win(const kss_profile& prof, const SPod& q_lds, const SPod& q0_lds,
                                                     const SimpleShard& L, int sl, int own, int pwv, int cand_w, int lo,
                                                     int start, uint32_t (&u)[12], const uint64_t* pused = nullptr,
                                                     SPort qp = SPort{}, uint64_t q0add = 0, const VolView* V = nullptr,
                                                     int vq = 0, int vp = 0) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t* sw = L.st + (size_t)sl * L.cap;
  const SPod q = q_lds;
  SPod q0;
#pragma unroll
  for (int k = 0; k < 3; k++) q0.creq[k] = q0_lds.creq[k];
  q0.cnz[0] = q0_lds.cnz[0];
  q0.cnz[1] = q0_lds.cnz[1];
  const bool scal = L.nsc > 0 && (DEF || ((prof.filter_enabled >> KSS_F_NODE_RESOURCES_FIT) & 1u));
  const int s = wv * pwv + lane;
  const bool extra = lane == pwv && cand_w >= 0;
  const bool mine = lane < pwv && s < own;
#pragma unroll
  for (int i = 0; i < 12; i++) u[i] = 0;
  if (mine || extra) {
    const int ns = extra ? cand_w : s;
    const uint32_t wd = sw[ns];
    DynRow r = shard_row(L, ns);
    if (extra) add_commit(r, q0);
    SVal e = DEF ? dyn_eval_def(q, wd, r) : dyn_eval(prof, q, wd, r);
    if constexpr (PI) pi_fix<DEF>(prof, e, pused[ns] | (extra ? q0add : 0ull), qp.conflict);
    if constexpr (VOL) e.f = (e.f == 0 && vol_infeasible(*V, ns, extra, vq, vp)) ? KSS_F_VOLUME_RESTRICTIONS : e.f;
    if (scal && e.f == 0 && scalar_short(L.sc, L.nsc, L.cap, ns, q_lds, extra, q0_lds)) e.f = KSS_F_NODE_RESOURCES_FIT;
    cv_put(L, extra ? L.cap + wv : s, e);
    win_acc(u, e.f == 0 && !extra, e.f == 0 && (extra || s != cand_w), lo + ns >= start ? 0 : 1, e);
  }
}

// the twelve window statistics over DPP lanes: counts summed, maxima kept
template <int CTRL, int ROWS>
__device__ __forceinline__ void dpp_win_step(uint32_t (&v)[12]) {
  uint32_t t[12];
#pragma unroll
  for (int i = 0; i < 12; i++) t[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[i], CTRL, ROWS, 0xF, false);
#pragma unroll
  for (int i = 0; i < 12; i++) v[i] = (i % 3 == 0) ? v[i] + t[i] : max(v[i], t[i]);
}

// inclusive prefix sum over the wave in DPP: row_shr 1, 2, 4, 8 scan each row of 16 lanes (lanes
// whose source falls outside the row add 0), row_bcast:15 adds row 0's total to row 1 and row 2's to
// row 3, row_bcast:31 adds rows 0-1's total to rows 2 and 3
template <int CTRL, int ROWS>
__device__ __forceinline__ void dpp_add2(uint32_t& a, uint32_t& b) {
  const uint32_t ta = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a, CTRL, ROWS, 0xF, false);
  const uint32_t tb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROWS, 0xF, false);
  a += ta;
  b += tb;
}
__device__ __forceinline__ void wave_incl_scan2(uint32_t& a, uint32_t& b) {
  dpp_add2<0x111, 0xF>(a, b);
  dpp_add2<0x112, 0xF>(a, b);
  dpp_add2<0x114, 0xF>(a, b);
  dpp_add2<0x118, 0xF>(a, b);
  dpp_add2<0x142, 0xA>(a, b);
  dpp_add2<0x143, 0xC>(a, b);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  uint32_t z = 0;
  wave_incl_scan2(v, z);
  return v;
}
// the maxima of two non-negative 32-bit values over the wave (uniform results)
__device__ __forceinline__ void wave_max2(uint32_t& a, uint32_t& b) {
  uint32_t t[2] = {a, b};
  auto step = [&](auto ctrl, auto rows) {
    constexpr int C = decltype(ctrl)::value, R = decltype(rows)::value;
    const uint32_t x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t[0], C, R, 0xF, false);
    const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t[1], C, R, 0xF, false);
    t[0] = max(t[0], x);
    t[1] = max(t[1], y);
  };
  step(std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xF>{});
  step(std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xF>{});
  step(std::integral_constant<int, 0x141>{}, std::integral_constant<int, 0xF>{});
  step(std::integral_constant<int, 0x140>{}, std::integral_constant<int, 0xF>{});
  step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{});
  step(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{});
  a = (uint32_t)__builtin_amdgcn_readlane((int)t[0], 63);
  b = (uint32_t)__builtin_amdgcn_readlane((int)t[1], 63);
}

// The cut shard: rank the feasible nodes of `part` (pod k+1's verdicts; the winner's slot takes
// its H1 verdict) in canonical order; d = the node of rank j, TT / NA = the maxima over ranks < j.
// Whole workgroup; results uniform.
template <bool PW>
__device__ __forceinline__ void win_cut_scan(SimpleHdr& H, const SimpleShard& L, int own, int lo, int start, int part,
                                             int j, int sub_s, int sub_h, int pwv, int& d, int& ptt, int& pna,
                                             bool maxima = true) {
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int iters = PW ? 1 : (own + nt - 1) / nt;
  int carry = 0, mt = 0, mn = 0;
  for (int it = 0; it < iters; it++) {
    const int s = PW ? wave * pwv + lane : it * nt + tid;
    const bool valid = PW ? (lane < pwv && s < own) : s < own;
    bool f = false;
    SVal e{0, 0, 0, 0, 0};
    if (valid && (part == 0 ? lo + s >= start : lo + s < start)) {
      e = cv_get(L, s == sub_s ? sub_h : s);
      f = e.f == 0;
    }
    const unsigned long long b = __ballot(f);
    if (lane == 0) H.cutc[it & 1][wave] = (int)__popcll(b);
    lds_barrier();
    int before = 0, tot = 0;
    for (int x = 0; x < nw; x++) {
      const int cx = H.cutc[it & 1][x];
      before += x < wave ? cx : 0;
      tot += cx;
    }
    const int rank = carry + before + (int)__popcll(b & ((1ull << lane) - 1ull));
    if (f && rank == j) H.win[6] = lo + s;
    mt = max(mt, (f && rank < j) ? e.tt : 0);
    mn = max(mn, (f && rank < j) ? e.na : 0);
    carry += tot;
  }
  ptt = 0;
  pna = 0;
  if (!maxima) {  // the cut segment's maxima cannot exceed the kept ones: only d is needed
    lds_barrier();  // H.win[6] written by its lane
    d = (int)H.win[6];
    return;
  }
  mt = (int)wave_red<OP_MAX>(mt);
  mn = (int)wave_red<OP_MAX>(mn);
  if (lane == 0) {
    H.cutm[wave][0] = mt;
    H.cutm[wave][1] = mn;
  }
  lds_barrier();
  for (int x = 0; x < nw; x++) {
    ptt = max(ptt, H.cutm[x][0]);
    pna = max(pna, H.cutm[x][1]);
  }
  d = (int)H.win[6];
}

// The window's statistics exchange (both per-wave and per-thread modes; PW: the best wave contributes
// its H1, else every wave's H1 set already accounts for the shard's candidate).  Pod k's AssumePod
// on the winner's slot is applied here (wave 0, lane-parallel) before the closing barrier.
// R = {winner key of pod k, kept count, max TT, max NA of pod k+1 over its kept nodes}; cs_out = pod
// k+1's cut segment (part * W + shard, -1: no cut), d_out = its dropped node (on the cut shard;
// -1 elsewhere).  start: this shard's split of pod k+1's node list (win_start).  False if the
// launch aborted.
template <bool PW, bool PI = false, bool VOL = false, typename Idle>
__device__ __forceinline__ bool simple_sync_win(SimpleHdr& H, int& parity, long long wkey, uint32_t (&u)[12], int W,
                                                int w, unsigned epoch, unsigned long long* gran, const XPeers& X,
                                                int* err, int per, int node_base, int lo, int own, const SPod& pk,
                                                bool commit, const SimpleShard& L, int kb, int k_find, int start,
                                                int pwv, long long (&R)[4], int& d_out, int& cs_out,
                                                KSS_GLOBAL unsigned long long* sp, Idle&& idle,
                                                uint64_t* pused = nullptr, uint64_t padd = 0, const VolView* V = nullptr, int vp = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (PW) {
    // one node (or the H1 re-evaluation) per lane: the four counts are ballot popcounts, the four
    // TaintToleration maxima (<= 64) ride as two packed 16-bit pairs, the NodeAffinity maxima alone:
    // six DPP chains instead of twelve
    uint32_t c4[4];
#pragma unroll
    for (int v = 0; v < 4; v++) c4[v] = (uint32_t)__popcll(__ballot(u[3 * v] != 0));
    uint32_t tp0 = u[1] | (u[4] << 16), tp1 = u[7] | (u[10] << 16), n0 = u[2], n1 = u[5], n2 = u[8], n3 = u[11];
    auto step = [&](auto ctrl, auto rows) {
      constexpr int C = decltype(ctrl)::value, R = decltype(rows)::value;
      dpp_pw_step<C, R>(tp0, n0, n1);
      dpp_pw_step<C, R>(tp1, n2, n3);
    };
    step(std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xF>{});
    step(std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xF>{});
    step(std::integral_constant<int, 0x141>{}, std::integral_constant<int, 0xF>{});
    step(std::integral_constant<int, 0x140>{}, std::integral_constant<int, 0xF>{});
    step(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{});
    step(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{});
#pragma unroll
    for (int v = 0; v < 4; v++) u[3 * v] = c4[v];
    u[1] = tp0 & 0xFFFFu;
    u[4] = tp0 >> 16;
    u[7] = tp1 & 0xFFFFu;
    u[10] = tp1 >> 16;
    u[2] = n0;
    u[5] = n1;
    u[8] = n2;
    u[11] = n3;
  } else {
    dpp_win_step<0xB1, 0xF>(u);
    dpp_win_step<0x4E, 0xF>(u);
    dpp_win_step<0x141, 0xF>(u);
    dpp_win_step<0x140, 0xF>(u);
    dpp_win_step<0x142, 0xA>(u);
    dpp_win_step<0x143, 0xC>(u);
  }
  if (sp && threadIdx.x == 0) sp[7] = wall_clock64();
  if (lane == 63) {  // the reduced values sit in lane 63
    H.red[parity][wave][0] = wkey;
#pragma unroll
    for (int i = 0; i < 12; i++) H.red[parity][wave][1 + i] = u[i];
  }
  lds_barrier();
  if (sp && threadIdx.x == 0) sp[8] = wall_clock64();
  idle();
  if (wave == 0) {
    // the shard: lane v < nw reads wave v's row, three DPP steps over the (at most 8) lanes
    const bool in = lane < nw;
    const long long* hv = H.red[parity][in ? lane : 0];
    const long long kv = in ? hv[0] : 0;
    long long best = kv;
    best = dpp_step<OP_MAX, 0xB1, 0xF>(best);
    best = dpp_step<OP_MAX, 0x4E, 0xF>(best);
    best = dpp_step<OP_MAX, 0x141, 0xF>(best);
    {
      const unsigned long long ub = (unsigned long long)best;
      best = (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(ub >> 32), 0) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ub, 0));
    }
    const bool me = PW ? (in && best != 0 && kv == best) : in;
    // per set (0: every wave's H0 values, 1: the best wave's H1 in place of its H0) the part a / b
    // counts and TaintToleration maxima as packed 16-bit pairs (both below 2^16: the exchange packs
    // them the same way), the NodeAffinity maxima alone: 8 words over three DPP steps
    kss_u16x2 pc[2], pt[2];
    uint32_t pn[4];
#pragma unroll
    for (int st = 0; st < 2; st++) {
      const int b = st == 0 ? 1 : (me ? 7 : 1);
      pc[st] = __builtin_bit_cast(kss_u16x2, in ? (uint32_t)hv[b] | ((uint32_t)hv[b + 3] << 16) : 0u);
      pt[st] = __builtin_bit_cast(kss_u16x2, in ? (uint32_t)hv[b + 1] | ((uint32_t)hv[b + 4] << 16) : 0u);
      pn[2 * st] = in ? (uint32_t)hv[b + 2] : 0u;
      pn[2 * st + 1] = in ? (uint32_t)hv[b + 5] : 0u;
    }
    auto cstep = [&](auto ctrl) {
      constexpr int C = decltype(ctrl)::value;
      uint32_t m[8];
#pragma unroll
      for (int st = 0; st < 2; st++) {
        m[st] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)__builtin_bit_cast(uint32_t, pc[st]), C, 0xF, 0xF, false);
        m[2 + st] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)__builtin_bit_cast(uint32_t, pt[st]), C, 0xF, 0xF, false);
      }
#pragma unroll
      for (int i = 0; i < 4; i++) m[4 + i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pn[i], C, 0xF, 0xF, false);
#pragma unroll
      for (int st = 0; st < 2; st++) {
        pc[st] = pc[st] + __builtin_bit_cast(kss_u16x2, m[st]);
        pt[st] = __builtin_elementwise_max(pt[st], __builtin_bit_cast(kss_u16x2, m[2 + st]));
      }
#pragma unroll
      for (int i = 0; i < 4; i++) pn[i] = max(pn[i], m[4 + i]);
    };
    cstep(std::integral_constant<int, 0xB1>{});
    cstep(std::integral_constant<int, 0x4E>{});
    cstep(std::integral_constant<int, 0x141>{});
    uint32_t t[12];
#pragma unroll
    for (int st = 0; st < 2; st++) {
      const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)__builtin_bit_cast(uint32_t, pc[st]), 0);
      const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)__builtin_bit_cast(uint32_t, pt[st]), 0);
      t[6 * st + 0] = c & 0xFFFFu;
      t[6 * st + 1] = x & 0xFFFFu;
      t[6 * st + 2] = (uint32_t)__builtin_amdgcn_readlane((int)pn[2 * st], 0);
      t[6 * st + 3] = c >> 16;
      t[6 * st + 4] = x >> 16;
      t[6 * st + 5] = (uint32_t)__builtin_amdgcn_readlane((int)pn[2 * st + 1], 0);
    }
    if (sp && lane == 0) sp[4] = wall_clock64();
    // every shard's packed values in the lane of that shard (W == 1: this shard in lane 0)
    uint32_t got[SX_CHUNKS][8];
    long long gbest = best;
    bool ok = true;
    if (W == 1) {
#pragma unroll
      for (int v = 0; v < 4; v++) {
        got[0][2 * v] = lane == 0 ? (t[3 * v] << 16) | t[3 * v + 1] : 0u;
        got[0][2 * v + 1] = lane == 0 ? t[3 * v + 2] : 0u;
      }
#pragma unroll
      for (int ch = 1; ch < SX_CHUNKS; ch++)
#pragma unroll
        for (int i = 0; i < 8; i++) got[ch][i] = 0;
    } else {
      const unsigned long long tag = (unsigned long long)epoch << 32;
      if (lane < SXW_VALS) {
        uint32_t x = (uint32_t)(unsigned long long)best;
        x = lane == 1 ? (uint32_t)((unsigned long long)best >> 32) : x;
#pragma unroll
        for (int v = 0; v < 4; v++) {
          x = lane == 2 + 2 * v ? ((t[3 * v] << 16) | t[3 * v + 1]) : x;
          x = lane == 3 + 2 * v ? t[3 * v + 2] : x;
        }
        xpub(X, gran, ((size_t)(epoch & 1) * W + w) * SXW_VALS + lane, tag | x);
      }
      const unsigned long long* base = gran + (size_t)(epoch & 1) * W * SXW_VALS;
      long long kbest = 0;
#pragma unroll
      for (int ch = 0; ch < SX_CHUNKS; ch++) {
#pragma unroll
        for (int i = 0; i < 8; i++) got[ch][i] = 0;
        if (ch * 64 >= W || !ok) continue;
        const int s = ch * 64 + lane;
        const bool valid = s < W;
        long long t0_ = 0;
        uint32_t k2[2] = {0, 0};
        for (unsigned spins = 0;; ++spins) {
          bool okp = true;
          unsigned long long g[SXW_VALS];
#pragma unroll
          for (int i = 0; i < SXW_VALS; i++)
            g[i] = __hip_atomic_load(base + (size_t)(valid ? s : 0) * SXW_VALS + i, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
          for (int i = 0; i < SXW_VALS; i++) okp &= !valid || (g[i] >> 32) == epoch;
          if (__all(okp)) {
            k2[0] = valid ? (uint32_t)g[0] : 0u;
            k2[1] = valid ? (uint32_t)g[1] : 0u;
#pragma unroll
            for (int i = 0; i < 8; i++) got[ch][i] = valid ? (uint32_t)g[2 + i] : 0u;
            break;
          }
          if (spin_expired(spins, t0_)) {
            if (lane == 0) {
              H.abort = 1;
              err_raise(err, 1);
            }
            ok = false;
            break;
          }
          spin_pause();
        }
        const long long kk = (long long)(((unsigned long long)k2[1] << 32) | k2[0]);
        kbest = kk > kbest ? kk : kbest;
      }
      gbest = wave_max_key(kbest, kb, node_base);
    }
    if (sp && lane == 0) sp[10] = wall_clock64();
    if (ok) {
      const int gl = key_node(gbest, node_base);
      // each lane's shard: H1 when the winner is one of its nodes
      uint32_t Fa[SX_CHUNKS], Fb[SX_CHUNKS], ta[SX_CHUNKS], tb[SX_CHUNKS], na_[SX_CHUNKS], nb_[SX_CHUNKS];
      uint32_t A = 0, B = 0, sa[SX_CHUNKS], sb[SX_CHUNKS], TA[SX_CHUNKS], TB[SX_CHUNKS];
#pragma unroll
      for (int ch = 0; ch < SX_CHUNKS; ch++) {
        const int s = ch * 64 + lane;
        const bool h1 = W > 1 ? (gl >= s * per && gl < s * per + per) : gbest != 0;
        const int o = h1 ? 4 : 0;
        Fa[ch] = got[ch][o] >> 16;
        ta[ch] = got[ch][o] & 0xFFFFu;
        na_[ch] = got[ch][o + 1];
        Fb[ch] = got[ch][o + 2] >> 16;
        tb[ch] = got[ch][o + 2] & 0xFFFFu;
        nb_[ch] = got[ch][o + 3];
        // per chunk: the inclusive scans of the part a / b counts and their totals
        sa[ch] = Fa[ch];
        sb[ch] = Fb[ch];
        TA[ch] = TB[ch] = 0;
        if (ch * 64 < W) {  // (uniform)
          wave_incl_scan2(sa[ch], sb[ch]);
          TA[ch] = (uint32_t)__builtin_amdgcn_readlane((int)sa[ch], 63);
          TB[ch] = (uint32_t)__builtin_amdgcn_readlane((int)sb[ch], 63);
        }
        A += TA[ch];
        B += TB[ch];
      }
      const uint32_t F = A + B, K = (uint32_t)k_find;
      uint32_t ftt = 0, fna = 0, cut_tt = 0, cut_na = 0;  // cut_*: the cut segment's maxima over all its feasible nodes
      int cut = -1, part = 0, j = 0;
      if (F <= K) {
#pragma unroll
        for (int ch = 0; ch < SX_CHUNKS; ch++) {
          ftt = max(ftt, max(ta[ch], tb[ch]));
          fna = max(fna, max(na_[ch], nb_[ch]));
        }
      } else {
        uint32_t ca = 0, cb = A;  // segments before this chunk
        unsigned long long hit = 0;
        int hit_ch = -1;
        uint32_t pre_hit = 0;
#pragma unroll
        for (int ch = 0; ch < SX_CHUNKS; ch++) {
          if (ch * 64 >= W) break;  // (uniform) no shard in this chunk
          const uint32_t pa = ca + sa[ch] - Fa[ch], pb = cb + sb[ch] - Fb[ch];
          ftt = max(ftt, pa + Fa[ch] <= K ? ta[ch] : 0u);
          fna = max(fna, pa + Fa[ch] <= K ? na_[ch] : 0u);
          ftt = max(ftt, pb + Fb[ch] <= K ? tb[ch] : 0u);
          fna = max(fna, pb + Fb[ch] <= K ? nb_[ch] : 0u);
          const bool cA = pa <= K && K < pa + Fa[ch], cB = pb <= K && K < pb + Fb[ch];
          const unsigned long long ba = __ballot(cA), bb = __ballot(cB);
          if (hit_ch < 0 && (ba | bb)) {
            const int l = __ffsll((long long)(ba ? ba : bb)) - 1;
            hit_ch = ch;
            hit = ba ? 0ull : 1ull;
            cut = ch * 64 + l;
            pre_hit = (uint32_t)__builtin_amdgcn_readlane((int)(ba ? pa : pb), l);
            cut_tt = (uint32_t)__builtin_amdgcn_readlane((int)(ba ? ta[ch] : tb[ch]), l);
            cut_na = (uint32_t)__builtin_amdgcn_readlane((int)(ba ? na_[ch] : nb_[ch]), l);
          }
          ca += TA[ch];
          cb += TB[ch];
        }
        part = (int)hit;
        j = (int)(K - pre_hit);
      }
      wave_max2(ftt, fna);
      // pod k's AssumePod on the winner's slot (before the closing barrier: the next pod's pass A
      // reads that row without a barrier of its own)
      if (commit && gbest != 0) {
        const int x = gl - lo;
        if (x >= 0 && x < own) simple_commit_lanes<PI, VOL>(L, pk, x, lane, pused, padd, V, vp);
      }
      if (lane == 0) {
        H.res[0] = gbest;
        H.win[0] = F;
        H.win[1] = ftt;
        H.win[2] = fna;
        H.win[3] = cut;
        H.win[4] = part;
        H.win[5] = j;
        H.win[10] = cut >= 0 && (cut_tt > ftt || cut_na > fna);  // the cut shard's partial maxima can matter
        if (sp) {
          sp[11] = wall_clock64();
          sp[14] = 1 + (cut == w ? 2 : 0) + (H.win[10] ? 4 : 0);
        }
      }
    }
  }
  parity ^= 1;
  lds_barrier();
  if (H.abort) return false;
  const long long F = H.win[0];
  const int cut = (int)H.win[3];
  long long mtt = H.win[1], mna = H.win[2], nf = F;
  int d = -1;
  cs_out = cut >= 0 ? (int)H.win[4] * W + cut : -1;
  if (cut >= 0) {
    nf = k_find;
    const bool need = H.win[10] != 0;
    const long long best = H.res[0];
    const int gl = key_node(best, node_base);
    const bool won = gl >= lo && gl < lo + own;
    const int sub_s = won ? gl - lo : -1;
    const int sub_h = PW ? L.cap + (won ? (gl - lo) / max(pwv, 1) : 0) : L.cap;
    const size_t e2 = 2 * (size_t)W * SXW_VALS + (size_t)(epoch & 1) * SXW_E2;
    if (cut == w) {  // uniform over the workgroup
      int cd = -1, ctt = 0, cna = 0;
      win_cut_scan<PW>(H, L, own, lo, start, (int)H.win[4], (int)H.win[5], sub_s, sub_h, pwv, cd, ctt, cna, need);
      d = cd;
      if (W == 1) {
        mtt = max(mtt, (long long)ctt);
        mna = max(mna, (long long)cna);
      } else if (need && threadIdx.x < 3) {
        const unsigned long long tag = (unsigned long long)epoch << 32;
        const uint32_t x = threadIdx.x == 0 ? (uint32_t)cd : (threadIdx.x == 1 ? (uint32_t)ctt : (uint32_t)cna);
        xpub(X, gran, e2 + threadIdx.x, tag | x);
      }
      if (sp && threadIdx.x == 0) sp[12] = wall_clock64();
    }
    if (W > 1 && need) {
      if (wave == 0) {
        const unsigned long long* b2 = gran + e2;
        long long t0_ = 0;
        for (unsigned spins = 0;; ++spins) {
          const unsigned long long g = __hip_atomic_load(b2 + min(lane, 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (__all((g >> 32) == epoch)) {
            if (lane < 3) H.win[7 + lane] = (long long)(uint32_t)g;
            break;
          }
          if (spin_expired(spins, t0_)) {
            if (lane == 0) {
              H.abort = 1;
              err_raise(err, 1);
            }
            break;
          }
          spin_pause();
        }
      }
      lds_barrier();
      if (H.abort) return false;
      mtt = max(mtt, H.win[8]);
      mna = max(mna, H.win[9]);
    }
  }
  R[0] = H.res[0];
  R[1] = nf;
  R[2] = mtt;
  R[3] = mna;
  d_out = d;
  return true;
}

// Pods [k0, k1) of the batch for shard w of one cluster (every pod commits).  `stat`
// holds the static words of those pods ([k - k0][N]).  On an exchange timeout the error
// word is set and the shard leaves without writing node state back.  PW: per-wave mode
// (simple_sync_pw; the caller checks that every shard's nodes fit it).  WIN: percentageOfNodesToScore
// < 100 (simple_sync_win): k_find = numFeasibleNodesToFind, cursor = the cluster's nextStartNodeIndex
// word (read at the start; written back at the end by the start shard, on a split grid by the first
// shard of every part from the start shard's granule).
// PI: the ports-and-images form (k_simple_pi).  The static words are k_static_pi's; sports
// holds the pods' NodePorts masks.  The UsedPorts column `pused` is node state like the rows: loaded
// with them, written back with them (so a chunked batch carries it from launch to launch through
// the same hand-off), committed with the row (simple_commit_lanes: same wave, same place relative
// to the barriers), read by pass A next to the row -- H1 with pod k's port_add ORed in, as H1 adds
// pod k's requests to the row.  The masks' ring is stored where the record ring is.
// VOL (with PI): the volumes form (k_simple_vol).  The static words are k_static_pi's with
// k_static_vol's VolumeBinding / VolumeZone verdicts; vl holds the pods' SVol records, the launch's
// constants and the node-state columns in HBM (packed before the batch's first launch, unpacked
// after its last: a chunked batch carries them from launch to launch as it carries UsedPorts).
// The used-rows / attached / limit columns are node state exactly like `pused`: loaded where it is
// loaded, written back where it is written back, committed by the lane next to its lane in
// simple_commit_lanes (same wave, same place relative to the barriers) and read by pass A where it
// is read -- H1 on the state after pod k's AssumePod, applied in registers (vol_assume).  The SVol
// ring is stored and read behind the same barriers as the SPort ring.  So what holds for `pused`
// above holds for them: no barrier of their own.
template <bool DEF, bool PW, bool WIN, bool PI = false, bool VOL = false>
__device__ __forceinline__ void simple_schedule(DevCluster c, const SPod* __restrict__ spods,
                                                const uint32_t* __restrict__ stat, const int32_t* __restrict__ ints,
                                                int k0, int k1, int32_t* chosen, PodMeta* meta, const kss_profile& prof,
                                                int W, int w, int cap, unsigned long long* gran, const XPeers& X,
                                                unsigned epoch0, int* err, unsigned long long* stamps, long long* smem,
                                                int k_find = 0, int32_t* cursor = nullptr,
                                                const SPort* __restrict__ sports = nullptr,
                                                const SVolLaunch* vl = nullptr) {
  static_assert(!VOL || PI, "the volumes form is a variant of the ports-and-images form");
  const int tid = threadIdx.x, nt = blockDim.x;
  SimpleHdr& H = *reinterpret_cast<SimpleHdr*>(smem);
  const SimpleShard L = shard_view(reinterpret_cast<uint8_t*>(smem) + sizeof(SimpleHdr), cap, c.n_scalar);
  SPort* const pring =
      PI ? reinterpret_cast<SPort*>(reinterpret_cast<uint8_t*>(smem) + (simple_lds_bytes(cap, c.n_scalar) + 15) / 16 * 16)
         : nullptr;
  uint64_t* const pused = PI ? reinterpret_cast<uint64_t*>(pring + RING) : nullptr;
  VolView VV{};
  if constexpr (VOL) VV = vol_view(reinterpret_cast<uint8_t*>(smem), cap, c.n_scalar, *vl);
  const VolView* const V = VOL ? &VV : nullptr;
  constexpr int NV = (int)(sizeof(SVol) / 16);
  const size_t N = (size_t)c.N;
  const int per = (c.N + W - 1) / W;
  const int lo = min(c.N, w * per), hi = min(c.N, lo + per), own = hi - lo;
  if (k1 <= k0) return;
  constexpr int NQ = (int)(sizeof(SPod) / 16);
  // prefetch distance: the record and static words of pod k + PD are loaded while pod k is
  // scheduled.  Per-wave mode has no barrier between a pod's end and the next pod's pass A, so
  // its prefetch stores land one pod earlier (behind two barriers) than the pass that reads them.
  constexpr int PD = PW ? 3 : 2;
  // shard rows, reciprocals, static words and records of pods k0 .. k0 + PD - 1 -> LDS
  handoff_acquire();
  for (int s = tid; s < own; s += nt) {
    const int n = lo + s;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int64_t A = c.alloc[k * N + n];
      L.r64[k * cap + s] = (double)A;
      L.r64[(3 + k) * cap + s] = (double)ld_ag(&c.requested[k * N + n]);
      L.inv[k * cap + s] = A > 0 ? 1.0 / (double)A : 0.0;
    }
    L.r64[6 * cap + s] = (double)ld_ag(&c.nonzero[n]);
    L.r64[7 * cap + s] = (double)ld_ag(&c.nonzero[N + n]);
    L.r32[s] = ld_ag(&c.pod_count[n]);
    L.r32[cap + s] = c.allowed_pods[n];
    for (int i = 0; i < L.nsc; i++) {
      L.sc[(size_t)i * cap + s] = c.alloc[(size_t)(3 + i) * N + n];
      L.sc[(size_t)(L.nsc + i) * cap + s] = ld_ag(&c.requested[(size_t)(3 + i) * N + n]);
    }
    for (int d = 0; d < PD && k0 + d < k1; d++) L.st[((k0 + d) % RING) * cap + s] = ld_ag(&stat[(size_t)d * N + lo + s]);
    if constexpr (PI) pused[s] = ld_ag(&c.port_used[n]);
    if constexpr (VOL) {
      VV.used[s] = ld_ag(&vl->used[n]);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        VV.att[h * cap + s] = ld_ag(&vl->att[h * N + n]);
        VV.lim[h * cap + s] = vl->lim[h * N + n];
      }
    }
  }
  for (int i = tid; i < min(k1 - k0, PD) * NQ; i += nt) {
    const int j = k0 + i / NQ;
    reinterpret_cast<uint4*>(L.ring + j % RING)[i % NQ] = reinterpret_cast<const uint4*>(spods + j)[i % NQ];
  }
  if constexpr (PI) {
    for (int i = tid; i < RING; i += nt) pring[i] = SPort{};  // (the prologue iteration reads the slot of pod k0 - 1)
    if constexpr (VOL) {
      for (int i = tid; i < RING * NV; i += nt) reinterpret_cast<uint4*>(VV.ring)[i] = make_uint4(0, 0, 0, 0);
      if (tid < SV_KEYS) const_cast<uint64_t*>(VV.keyrows)[tid] = vl->keyrows[tid];
    }
    __syncthreads();
    for (int i = tid; i < min(k1 - k0, PD); i += nt) pring[(k0 + i) % RING] = sports[k0 + i];
    if constexpr (VOL) {
      for (int i = tid; i < min(k1 - k0, PD) * NV; i += nt)
        reinterpret_cast<uint4*>(VV.ring + (k0 + i / NV) % RING)[i % NV] =
            reinterpret_cast<const uint4*>(vl->svols + k0 + i / NV)[i % NV];
    }
  }
  if (tid == 0) H.abort = 0;
  __syncthreads();
  // the window (WIN).  A shard splits its slots at a pod's start node s into part a (node >= s) and
  // part b by `wsl`: s itself on the shard holding s (the start shard, wss), past its last node on
  // shards before it (every node in part b), its first node on shards after it (every node in part
  // a).  wsx: s, on the start shard.  wcs: pod k's cut segment (-1 none), wd: its dropped node, on
  // the cut shard (pass B).  Pod k0 starts at the cursor word.
  const int cur0 = WIN && cursor && c.N > 0 ? (int)(((long long)ld_ag(cursor) % c.N + c.N) % c.N) : 0;
  auto win_start = [&](int sh, int x) { return w < sh ? lo + own : (w > sh ? lo : x); };
  int wss = WIN ? min(cur0 / max(per, 1), W - 1) : 0, wsx = cur0;
  int wsl = win_start(wss, cur0), wcs = -1, wd = -1;

  KSS_GLOBAL const uint32_t* gstat = gp(stat);
  KSS_GLOBAL const uint4* gspod = gp(reinterpret_cast<const uint4*>(spods));
  KSS_GLOBAL unsigned long long* gstamps = gp(stamps);
  KSS_GLOBAL const uint4* gsport = gp(reinterpret_cast<const uint4*>(sports));
  uint4 pfp = make_uint4(0, 0, 0, 0);  // PI: the prefetched port masks of pod k+PD
  KSS_GLOBAL const uint4* gsvol = gp(reinterpret_cast<const uint4*>(VOL ? vl->svols : nullptr));
  uint4 pfv = make_uint4(0, 0, 0, 0);  // VOL: a quarter of its SVol (prefetch lanes 0 .. NV - 1)
  long long st[6], R[4] = {0, 0, 0, 0};
  // the outcome of pod pend_k, not yet stored (thread out_tid of shard w_off)
  const int out_tid = (nt >> 6) > 1 ? 64 : 0;
  const bool defer_out = PW && (nt >> 6) > 1;
  PodMeta pend{};
  int pend_k = -1;
  auto store_pending = [&]() {
    if (pend_k < 0) return;
    if (chosen) gp(chosen)[pend_k] = pend.chosen;
    if (meta) {
      KSS_GLOBAL PodMeta* mm = gp(meta) + pend_k;
      mm->chosen = pend.chosen;
      mm->n_feasible = pend.n_feasible;
      mm->scored = pend.scored;
      mm->status = pend.status;
      mm->best_total = pend.best_total;
    }
    pend_k = -1;
  };
  int parity = 0, sub_s = -1;  // slot whose pass-B values are the H1 ones (the previous winner)
  int sub_h = cap;             // ... and the cv slot holding them
  unsigned epoch = epoch0;  // granule tags above every tag an earlier launch left (split grids)
  const int nwave = nt >> 6;
  const int lane = tid & 63, wv = tid >> 6;
  const int pwv = (own + nwave - 1) / nwave;  // per-wave mode: the wave's node slots (<= PW_LANES)
  const int kb = key_bits(prof, c.N);  // 32-bit key reductions when the keys fit (0: 64-bit)
  // prefetch lanes: every wave but wave 0 (readfirstlane: a wave-uniform, scalar branch).
  // Per-wave mode with 3+ waves: the last wave (fewest slots) alone prefetches, so the first
  // prefetch wave reaches the statistics barrier with the others (r8u A/B, C2: 303.3 / 303.6 k
  // against 301.6 / 301.5 k pods/s)
  const int pf_w0 = (PW && nwave >= 3) ? nwave - 1 : 1;
  const bool pf_wave = nwave == 1 || __builtin_amdgcn_readfirstlane(tid >> 6) >= pf_w0;
  uint4 pfq = make_uint4(0, 0, 0, 0);  // prefetched record / static words of pod k+PD, live across the loop
  uint32_t pfw[PF_MAX];
#pragma unroll
  for (int j = 0; j < PF_MAX; j++) pfw[j] = 0;
  const int pf_lane = nwave == 1 ? tid : tid - 64 * pf_w0, pf_n = nwave == 1 ? nt : nt - 64 * pf_w0;
  const int pf_per = (own + pf_n - 1) / pf_n;  // static words per prefetch lane (<= PF_MAX)
  // k = k0 - 1 is the prologue: pass A of pod k0 and the exchange of its statistics
  for (int k = k0 - 1; k < k1; k++) {
    // diagnostic phase stamps (KSS_STAMPS_FILE): lane 0 of every shard, the first pods
    KSS_GLOBAL unsigned long long* sp = (stamps && k >= k0 && k - k0 < KSS_NSTAMP_PODS / 2)
                                            ? gstamps + (size_t)w * 8 * KSS_NSTAMP_PODS + (size_t)(k - k0) * 16
                                            : nullptr;
    if (sp && tid == 0) sp[0] = wall_clock64();
    if (sp && tid == 64) sp[9] = wall_clock64();  // wave 1's start of the pod
    const SPod& pk = L.ring[(k + RING) % RING];
    // pod k+PD: record and static words -> registers now, -> their ring slots at the end
    // Only the prefetch waves (all but wave 0, unless there is one wave) issue these loads:
    // vmcnt is per wave and counts stores too, so wave 0 — which publishes granules and
    // writes the outcomes — never waits on an HBM prefetch, and the prefetch waves never
    // wait on a store.
    // The branch is wave-uniform and every load inside it is unconditional (clamped
    // indices), so the compiler's wait for these registers stays on the prefetch path.
    const bool pf_on = pf_wave && k >= k0 && k + PD < k1 && own > 0;
    auto prefetch = [&]() {
      if (pf_on) {
        KSS_GLOBAL const uint4& src = gspod[(size_t)(k + PD) * NQ + min(pf_lane, NQ - 1)];
        pfq = make_uint4(src.x, src.y, src.z, src.w);
        if constexpr (PI) {  // (every prefetch lane the same 16 bytes)
          KSS_GLOBAL const uint4& ps = gsport[(size_t)(k + PD)];
          pfp = make_uint4(ps.x, ps.y, ps.z, ps.w);
        }
        if constexpr (VOL) {
          KSS_GLOBAL const uint4& vs = gsvol[(size_t)(k + PD) * NV + min(pf_lane, NV - 1)];
          pfv = make_uint4(vs.x, vs.y, vs.z, vs.w);
        }
#pragma unroll
        for (int j = 0; j < PF_MAX; j++)
          if (j < pf_per) pfw[j] = ld_ag(&gstat[(size_t)(k + PD - k0) * N + lo + min(j * pf_n + pf_lane, own - 1)]);
      }
    };
    auto ring_store = [&]() {  // lanes past the end rewrite the last element with its own value
      if (pf_on) {
        reinterpret_cast<uint4*>(L.ring + (k + PD) % RING)[min(pf_lane, NQ - 1)] = pfq;
        if constexpr (PI) {
          if (pf_lane == 0) *reinterpret_cast<uint4*>(pring + (k + PD) % RING) = pfp;
        }
        if constexpr (VOL) {
          if (pf_lane < NV) reinterpret_cast<uint4*>(VV.ring + (k + PD) % RING)[pf_lane] = pfv;
        }
#pragma unroll
        for (int j = 0; j < PF_MAX; j++)
          if (j < pf_per) L.st[((k + PD) % RING) * cap + min(j * pf_n + pf_lane, own - 1)] = pfw[j];
      }
    };
    // issued here; per-wave mode with several waves stores them into the ring while wave 0
    // exchanges (simple_sync_pw's idle hook: slot (k + PD) % RING held pod k - 1, whose last
    // reader finished before the statistics barrier), then this pod's HBM stores follow, after
    // every wait on a load of this wave
    prefetch();
    auto prefetch_idle = [&]() {
      if (defer_out) {
        ring_store();
        if (tid == out_tid) store_pending();  // the previous pod's outcome
      }
    };
    // pass B: NormalizeScore, weights, shard-best selectHost key of pod k
    const long long nf = R[1];
    const int max_tt = (int)R[2], max_na = (int)R[3];
    const bool scored = nf > 1;
    long long best = 0;
    int cand = -1;  // the candidate slot whose H1 pass A evaluates (the shard's / the wave's best)
    const bool keys = k >= k0 && pk.status == 0 && nf > 0;
    const float rtt = __builtin_amdgcn_rcpf((float)max(max_tt, 1));
    const float rna = __builtin_amdgcn_rcpf((float)max(max_na, 1));
    if constexpr (PW) {
      // every slot's five values read at once and its key computed whatever the verdict, then
      // selected: one LDS round trip per slot, no exec-mask region; the wave's best by DPP
      const int s = wv * pwv + lane;
      if (keys && lane < pwv && s < own) {
        SVal e = cv_get(L, s == sub_s ? sub_h : s);
        const long long ilk = PI ? pi_key_add<DEF>(prof, e, scored) : 0ll;
        const long long key = simple_key(prof, e, scored, max_tt, rtt, max_na, rna, (uint32_t)(c.node_base + lo + s)) + ilk;
        bool kept = true;
        if (WIN && wcs >= 0) {  // the node's segment before the cut segment, or before d inside it
          const int n = lo + s, seg = (n >= wsl ? 0 : W) + w;
          kept = seg < wcs || (seg == wcs && n < wd);
        }
        best = (e.f == 0 && kept) ? key : 0;
      }
      if (sp && tid == 0) sp[1] = wall_clock64();
      best = wave_max_key(best, kb, c.node_base);
      if (sp && tid == 0) sp[2] = wall_clock64();
    } else {
      if (k >= k0) {
        if (keys) {
          for (int s = tid; s < own; s += nt) {
            SVal e = cv_get(L, s == sub_s ? sub_h : s);
            const long long ilk = PI ? pi_key_add<DEF>(prof, e, scored) : 0ll;
            const long long key =
                simple_key(prof, e, scored, max_tt, rtt, max_na, rna, (uint32_t)(c.node_base + lo + s)) + ilk;
            bool kept = true;
            if (WIN && wcs >= 0) {
              const int n = lo + s, seg = (n >= wsl ? 0 : W) + w;
              kept = seg < wcs || (seg == wcs && n < wd);
            }
            best = (e.f == 0 && kept && key > best) ? key : best;
          }
        }
        if (sp && tid == 0) sp[1] = wall_clock64();
        long long b[1] = {best};
        const int op[1] = {OP_MAX};
        block_red(H, parity, b, op);
        parity ^= 1;
        best = b[0];
        if (sp && tid == 0) sp[2] = wall_clock64();
      }
    }
    cand = best ? (int)(0xFFFFFFFFu - (uint32_t)(unsigned long long)best) - c.node_base - lo : -1;
    // pass A: pod k+1 before pod k's commit, and on the candidate after it
    const SPod& qn = L.ring[(k + 1) % RING];
    const int sln = (k + 1) % RING;
    // PI: pod k's port_add (its commit, and H1 of pod k+1) and pod k+1's masks, wave-uniform LDS
    // reads, here and not at the top: like qn, pod k+1's slot is behind pass B's barrier (not PW)
    const uint64_t pk_add = PI ? pring[(k + RING) % RING].add : 0ull;
    const SPort qnp = PI ? pring[(k + 1) % RING] : SPort{};
    const int vqn = (k + 1) % RING, vpk = (k + RING) % RING;  // VOL: the SVol ring slots of pod k+1 and pod k
    if constexpr (WIN) {
      // pod k+1 starts where pod k's window stopped (its dropped node, on the cut shard), else
      // where pod k started
      if (k >= k0 && wcs >= 0) {
        wss = wcs % W;
        if (w == wss) wsx = wd;
        wsl = win_start(wss, wd);
      }
      uint32_t u[12];
      if (k + 1 < k1) {
        if constexpr (PW) simple_pass_a_pw_win<DEF, PI, VOL>(prof, qn, pk, L, sln, own, pwv, cand, lo, wsl, u, pused, qnp, pk_add, V, vqn, vpk);
        else simple_pass_a_win<DEF, PI, VOL>(prof, qn, pk, L, sln, own, cand, lo, wsl, u, pused, qnp, pk_add, V, vqn, vpk);
      } else {
#pragma unroll
        for (int i = 0; i < 12; i++) u[i] = 0;
      }
      if (sp && tid == 0) sp[3] = wall_clock64();
      if (!simple_sync_win<PW, PI, VOL>(H, parity, best, u, W, w, ++epoch, gran, X, err, per, c.node_base, lo, own, pk, k >= k0,
                                   L, kb, k_find, wsl, pwv, R, wd, wcs, sp, prefetch_idle, pused, pk_add, V, vpk))
        return;
    } else if constexpr (PW) {
      uint32_t u[6];
      if (k + 1 < k1) {
        simple_pass_a_pw<DEF, PI, VOL>(prof, qn, pk, L, sln, own, pwv, cand, u, pused, qnp, pk_add, V, vqn, vpk);
      } else {
#pragma unroll
        for (int i = 0; i < 6; i++) u[i] = 0;
      }
      if (sp && tid == 0) sp[3] = wall_clock64();
      if (!simple_sync_pw<PI, VOL>(H, parity, best, u, W, w, ++epoch, gran, X, err, per, c.node_base, lo, own, pk, k >= k0, L, kb,
                              R, sp, prefetch_idle, pused, pk_add, V, vpk))
        return;
    } else {
      if (k + 1 < k1) {
        simple_pass_a<DEF, PI, VOL>(prof, qn, pk, L, sln, own, cand, st, pused, qnp, pk_add, V, vqn, vpk);
      } else {
#pragma unroll
        for (int i = 0; i < 6; i++) st[i] = 0;
      }
      if (sp && tid == 0) sp[3] = wall_clock64();
      if (!simple_sync(H, parity, best, st, W, w, ++epoch, gran, X, err, per, c.node_base, kb, R, sp)) return;
    }
    if (sp && tid == 0) sp[5] = wall_clock64();
    if (k >= k0) {
      const long long K = R[0];
      const int x = K ? (int)(0xFFFFFFFFu - (uint32_t)(unsigned long long)K) - c.node_base : -1;
      // AssumePod on the winner's shard (per-wave mode: done inside the sync); pass B of pod
      // k+1 takes that slot's H1 values: cv slot cap (cap + the slot's wave in per-wave mode)
      const bool won = x >= lo && x < hi;
      sub_s = won ? x - lo : -1;
      sub_h = PW ? cap + (won ? (x - lo) / max(pwv, 1) : 0) : cap;
      if (!PW && !WIN && won && tid < 64) simple_commit_lanes<PI, VOL>(L, pk, x - lo, tid, pused, pk_add, V, vpk);
      // the HBM-only class / term counts are applied after the launch (k_counts): nothing in
      // this loop reads them
    }
    if (!defer_out) ring_store();
    // every part keeps the outcomes.  Their HBM stores are issued off wave 0 (whose vmcnt stays
    // free for the exchange polls); with several waves in per-wave mode they are held in
    // registers and issued while the NEXT pod's exchange runs (store_pending in the idle hook,
    // ahead of that wave's prefetch loads), so no wait on a store lands on the pod chain
    if (k >= k0 && w == X.w_off && tid == out_tid) {
      const long long K = R[0];
      const int x = K ? (int)(0xFFFFFFFFu - (uint32_t)(unsigned long long)K) - c.node_base : -1;
      pend.chosen = K ? x + c.node_base : -1;
      pend.n_feasible = (int)nf;
      pend.scored = (K && scored) ? 1 : 0;
      pend.status = pk.status != 0 ? (pk.status == KSS_PF_ERROR ? 3 : 2) : (nf == 0 ? 1 : 0);
      pend.best_total = pend.scored ? (int64_t)((unsigned long long)K >> 32) : 0;
      pend_k = k;
      if (!defer_out) store_pending();
    }
    if (sp && tid == 0) sp[6] = wall_clock64();
  }
  if (tid == out_tid) store_pending();  // the last pod's outcome
  // nextStartNodeIndex after the last pod: the start shard of the pod after it writes it (the last
  // iteration's pass A, for no pod, already moved the start past the last pod's cut)
  if constexpr (WIN) {
    if (X.n <= 1) {
      if (cursor && w == wss && tid == 0) st_ag(cursor, (int32_t)wsx);
    } else {
      // Split grid: every part has a cursor word of its own, read by its next chunk launch and its
      // next run, and only the start shard knows s.  It publishes s as one more epoch-tagged
      // granule into every part's inbox (SXW_CUR, behind the cut granules); the first shard of
      // each part polls its local copy and stores the part's word.  One granule per launch and
      // inbox half: a part one chunk ahead publishes its next cursor into the OTHER half (the
      // halves alternate by chunk), and this address is written again only two chunks later, at
      // the end of a launch whose per-pod exchanges need every part -- so behind this part's poll,
      // which precedes that launch in its stream.  The tag is above every tag the loop used.
      const size_t co = xcd_ctr_off<true>(W);  // (a split grid is never XCD-local: the same words, behind the cut granules)
      ++epoch;
      if (w == wss && tid == 0) xpub(X, gran, co, ((unsigned long long)epoch << 32) | (uint32_t)wsx);
      if (w == X.w_off && tid == 0) {
        long long t0_ = 0;
        for (unsigned spins = 0;; ++spins) {
          const unsigned long long g = __hip_atomic_load(gran + co, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((g >> 32) == epoch) {
            if (cursor) st_ag(cursor, (int32_t)(uint32_t)g);
            break;
          }
          if (spin_expired(spins, t0_)) {
            H.abort = 1;
            err_raise(err, 1);
            break;
          }
          spin_pause();
        }
      }
    }
  }
  // node state back to HBM
  __syncthreads();
  if (WIN && X.n > 1 && H.abort) return;  // as every exchange timeout: no node state written back
  for (int s = tid; s < own; s += nt) {
    const int n = lo + s;
#pragma unroll
    for (int r = 0; r < 3; r++) st_ag(&c.requested[(size_t)r * N + n], (int64_t)L.r64[(3 + r) * cap + s]);
    st_ag(&c.nonzero[n], (int64_t)L.r64[6 * cap + s]);
    st_ag(&c.nonzero[N + n], (int64_t)L.r64[7 * cap + s]);
    st_ag(&c.pod_count[n], L.r32[s]);
    for (int i = 0; i < L.nsc; i++) st_ag(&c.requested[(size_t)(3 + i) * N + n], L.sc[(size_t)(L.nsc + i) * cap + s]);
    if constexpr (PI) st_ag(&c.port_used[n], pused[s]);
    if constexpr (VOL) {
      st_ag(&vl->used[n], VV.used[s]);
      st_ag(&vl->att[n], VV.att[s]);
      st_ag(&vl->att[N + n], VV.att[cap + s]);
    }
  }
  handoff_release();
}

// ---------------------------------------------------------------------------
// The flat exchange of the table loop (k_simple_tab_flat): every WAVE publishes its own entry,
// and wave 0 of every shard sweeps the entries of all W x nwave waves.  simple_sync_pw reduces
// the waves of a shard first ("the best wave contributes H1, every other wave H0") and
// simple_exchange then the shards ("the winner's shard contributes H1, every other H0"): together
// "the winner's wave contributes H1, every other wave H0", which one sweep over the waves
// computes by itself -- without the LDS round trip, the barrier wait and wave 0's combine
// between a wave's statistics and its publish.
// An entry is SXF_VALS granules {epoch << 32 | 32-bit payload}:
//   0  the wave's best key, compressed (key_compress: the host admits the form only with key_bits > 0)
//   1  nf0 | tt0 << 8 | nf1 << 16 | tt1 << 24   (counts <= PW_LANES per wave, raw TaintToleration <= 64)
//   2  na0        3  na1
// at granule (parity * E + e) * SXF_VALS + field, e = shard * nwave + wave, E = W * nwave.
// ---------------------------------------------------------------------------
constexpr int SXF_VALS = 4;       // granules per wave entry
constexpr int SXF_LOADS = 8;      // sweep loads per lane: SXF_VALS * E <= 64 * SXF_LOADS
constexpr int SXF_MAX_E = 64 * SXF_LOADS / SXF_VALS;  // 128 entries (host-checked: flat_exchange_ok)
static_assert(PW_LANES < 256, "granule 1 packs a wave's feasible counts in 8 bits");

// The entry of the wave that owns node gl (index relative to node_base) on W shards of `per`
// nodes (the last ones shorter or empty) with nwave waves each: wave v of a shard of `own` nodes
// owns its slots [v * pwv, v * pwv + pwv), pwv = ceil(own / nwave) (simple_schedule_tab's split).
__host__ __device__ constexpr int flat_entry(int gl, int per, int N, int nwave) {
  const int sh = gl / per, lo = sh * per;
  const int own = (N - lo < per ? N - lo : per);
  const int pwv = (own + nwave - 1) / nwave;
  return sh * nwave + (gl - lo) / pwv;
}
// The nodes of entry e as first node << 8 | count (count <= PW_LANES; 0 for an empty wave or a
// shard past W): what the sweep's lanes hold for their entries, computed once per launch, so
// that no division stands between the winner's key and the statistics on the per-pod chain.
__host__ __device__ constexpr uint32_t flat_entry_range(int e, int per, int N, int W, int nwave) {
  const int sh = e / nwave, v = e - sh * nwave;
  if (sh >= W) return 0u;
  const int lo = sh * per;
  const int own = N - lo < 0 ? 0 : (N - lo < per ? N - lo : per);
  const int pwv = (own + nwave - 1) / nwave;
  const int a = v * pwv < own ? v * pwv : own, b = a + pwv < own ? a + pwv : own;
  return ((uint32_t)(lo + a) << 8) | (uint32_t)(b - a);
}
__host__ __device__ constexpr bool flat_range_holds(uint32_t r, int gl) {
  return (uint32_t)(gl - (int)(r >> 8)) < (r & 0xFFu);  // (gl = -1, no winner: in no range)
}
// every node lies in the range of its entry and in no other one
__host__ __device__ constexpr bool flat_ranges_agree(int N, int W, int nwave) {
  const int per = (N + W - 1) / W;
  for (int gl = 0; gl < N; gl++)
    for (int e = 0; e < W * nwave; e++)
      if (flat_range_holds(flat_entry_range(e, per, N, W, nwave), gl) != (e == flat_entry(gl, per, N, nwave))) return false;
  for (int e = 0; e < W * nwave; e++)
    if (flat_range_holds(flat_entry_range(e, per, N, W, nwave), -1)) return false;
  return true;
}
static_assert(flat_ranges_agree(377, 3, 2) && flat_ranges_agree(378, 3, 2) && flat_ranges_agree(3, 3, 3) &&
                  flat_ranges_agree(10, 2, 3) && flat_ranges_agree(9, 2, 3) && flat_ranges_agree(5, 4, 2) &&
                  flat_ranges_agree(128, 64, 2) && flat_ranges_agree(1007, 2, 8),
              "flat_entry_range: the lanes' ranges are flat_entry's mapping");
// a last shard one node short: 377 nodes on 3 shards x 2 waves, shard 2 holds 125 (63 + 62)
static_assert(flat_entry(376, 126, 377, 2) == 5 && flat_entry(314, 126, 377, 2) == 4 && flat_entry(315, 126, 377, 2) == 5 &&
                  flat_entry(251, 126, 377, 2) == 3 && flat_entry(252, 126, 377, 2) == 4,
              "flat_entry: last shard one node short");
// shards of one node: the node is wave 0's, waves 1.. are empty
static_assert(flat_entry(0, 1, 3, 3) == 0 && flat_entry(1, 1, 3, 3) == 3 && flat_entry(2, 1, 3, 3) == 6,
              "flat_entry: shards of one node");
// own not divisible by nwave: 10 nodes on 2 shards x 3 waves, 5 per shard as 2 + 2 + 1
static_assert(flat_entry(1, 5, 10, 3) == 0 && flat_entry(2, 5, 10, 3) == 1 && flat_entry(4, 5, 10, 3) == 2 &&
                  flat_entry(5, 5, 10, 3) == 3 && flat_entry(9, 5, 10, 3) == 5,
              "flat_entry: own not divisible by nwave");
// ... and a short last shard whose own is not divisible either: 9 nodes, shard 1 holds 4 as 2 + 2 + 0
static_assert(flat_entry(8, 5, 9, 3) == 4 && flat_entry(6, 5, 9, 3) == 3, "flat_entry: short last shard, empty last wave");

// simple_sync_pw's place in the table loop with the flat exchange.  Every wave: its statistics
// (wave_red_stats_pw), its entry published by lanes 0..3, then its candidate to H.red for the
// refresh (idle) and the statistics barrier -- which now overlaps the stores' way to the L2
// instead of preceding the publish.  Wave 0 sweeps; the closing barrier hands H.res to the others.
// No commit here (simple_schedule_tab's owner wave commits after the closing barrier).
// R = {winner key, nf, max TT, max NA of the next pod}.  False if the launch aborted.
template <typename Idle>
__device__ __forceinline__ bool simple_sync_flat(SimpleHdr& H, int& parity, long long wbest, uint32_t (&u)[6], int W,
                                                 int w, unsigned epoch, unsigned long long* gran, const XPeers& X,
                                                 int* err, int node_base, int kb, const uint32_t (&er)[SXF_LOADS],
                                                 long long (&R)[4], KSS_GLOBAL unsigned long long* sp, Idle&& idle) {
  wave_red_stats_pw(u);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int E = W * nw;
  const unsigned long long tag = (unsigned long long)epoch << 32;
  if (sp && threadIdx.x == 0) sp[7] = wall_clock64();
  if (lane < SXF_VALS) {
    uint32_t x = key_compress(wbest, kb, node_base);
    x = lane == 1 ? (u[0] | (u[1] << 8) | (u[3] << 16) | (u[4] << 24)) : x;
    x = lane == 2 ? u[2] : x;
    x = lane == 3 ? u[5] : x;
    xpub(X, gran, ((size_t)(epoch & 1) * E + (size_t)w * nw + wave) * SXF_VALS + lane, tag | x);
  }
  // stamps: 4 wave 0 published (the two-level form's slot 4 is its one publish too), 10 / 11 waves 1 / 2 did
  if (sp && threadIdx.x == 0) sp[4] = wall_clock64();
  if (sp && (threadIdx.x == 64 || threadIdx.x == 128)) sp[9 + (threadIdx.x >> 6)] = wall_clock64();
  if (lane == 0) H.red[parity][wave][0] = wbest;
  lds_barrier();
  if (sp && threadIdx.x == 0) sp[8] = wall_clock64();
  idle();
  if (wave == 0) {
    if (sp && lane == 0) sp[15] = wall_clock64();  // sweep start (slot 15 > 0 marks the flat form)
    const int G = SXF_VALS * E, nld = (G + 63) >> 6;
    const unsigned long long* base = gran + (size_t)(epoch & 1) * G;
    uint32_t got[SXF_LOADS];
    bool done = false;
    long long t0_ = 0;
    for (unsigned spins = 0;; ++spins) {
      bool ok = true;
      unsigned long long g[SXF_LOADS];
      // every load issued before the first is looked at (lanes past the end read granule 0)
#pragma unroll
      for (int i = 0; i < SXF_LOADS; i++) {
        g[i] = tag;
        if (i < nld) {
          const int idx = i * 64 + lane;
          g[i] = __hip_atomic_load(base + (idx < G ? idx : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
#pragma unroll
      for (int i = 0; i < SXF_LOADS; i++) {
        ok &= (g[i] >> 32) == epoch;
        got[i] = i * 64 + lane < G ? (uint32_t)g[i] : 0u;
      }
      if (__all(ok)) {
        done = true;
        break;
      }
      if (spin_expired(spins, t0_)) break;
      spin_pause();
    }
    if (!done) {
      if (lane == 0) {
        H.abort = 1;
        err_raise(err, 1);
      }
    } else {
      // lane l holds field l & 3 of the entries i * 16 + (l >> 2): the key lanes' maximum, then the wave's
      const int field = lane & 3;
      uint32_t k = 0;
#pragma unroll
      for (int i = 0; i < SXF_LOADS; i++) k = max(k, got[i]);
      k = field == 0 ? k : 0u;
#define KSS_KSTEP(CTRL, ROWS) k = max(k, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)k, CTRL, ROWS, 0xF, false))
      KSS_KSTEP(0xB1, 0xF);
      KSS_KSTEP(0x4E, 0xF);
      KSS_KSTEP(0x141, 0xF);
      KSS_KSTEP(0x140, 0xF);
      KSS_KSTEP(0x142, 0xA);
      KSS_KSTEP(0x143, 0xC);
#undef KSS_KSTEP
      k = (uint32_t)__builtin_amdgcn_readlane((int)k, 63);
      const long long best = key_expand(k, kb, node_base);
      // the winner's wave contributes its H1, every other wave its H0: er[i], the nodes of this
      // lane's entry i * 16 + (lane >> 2) (flat_entry_range), holds the winner's node or not
      const int gl = k ? (int)(((1u << kb) - 1u) - (k & ((1u << kb) - 1u))) : -1;
      uint32_t nf = 0, tt = 0, na = 0;
#pragma unroll
      for (int i = 0; i < SXF_LOADS; i++) {
        const bool h1 = flat_range_holds(er[i], gl);
        const uint32_t v = got[i];
        const uint32_t b = h1 ? v >> 16 : v;  // field 1: {nf, tt} of the hypothesis
        nf += field == 1 ? (b & 0xFFu) : 0u;
        tt = max(tt, field == 1 ? ((b >> 8) & 0xFFu) : 0u);
        na = max(na, (field == 2 && !h1) || (field == 3 && h1) ? v : 0u);
      }
#define KSS_FSTEP(CTRL, ROWS)                                                                      \
  {                                                                                                \
    const uint32_t a_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)nf, CTRL, ROWS, 0xF, false); \
    const uint32_t b_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tt, CTRL, ROWS, 0xF, false); \
    const uint32_t c_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)na, CTRL, ROWS, 0xF, false); \
    nf += a_;                                                                                      \
    tt = max(tt, b_);                                                                              \
    na = max(na, c_);                                                                              \
  }
      KSS_FSTEP(0xB1, 0xF)
      KSS_FSTEP(0x4E, 0xF)
      KSS_FSTEP(0x141, 0xF)
      KSS_FSTEP(0x140, 0xF)
      KSS_FSTEP(0x142, 0xA)
      KSS_FSTEP(0x143, 0xC)
#undef KSS_FSTEP
      if (lane == 63) {
        H.res[0] = best;
        H.res[1] = nf;
        H.res[2] = tt;
        H.res[3] = na;
      }
    }
  }
  parity ^= 1;
  lds_barrier();
  if (H.abort) return false;
#pragma unroll
  for (int i = 0; i < 4; i++) R[i] = H.res[i];
  return true;
}

// simple_schedule<true, true, false> with the shape table (k_simple_tab): the default profile,
// per-wave mode with at least two waves, no window, no extended resources, and a batch of at most
// KSS_MAX_SHAPES resource shapes (SPod::shape).  The state-dependent part of an evaluation --
// the NodeResourcesFit verdict and the Fit / BalancedAllocation scores -- depends on the node's
// row and the pod's shape only, and a commit changes one row.  So the shard keeps
//   T[c][s] = dyn_eval_def(shape c, row s), packed (shape_pack), for every shape c and slot s,
// and a pod reads its values instead of evaluating them:
//   pass B of pod k      T[shape(k)][s] and the pod's static word -> the selectHost key;
//   statistics of k+1    H0 from T[shape(k+1)][s]; H1 (the wave's candidate with pod k added) needs
//                        the filter verdict only: the pod count and three resource comparisons;
//   refresh              while wave 0 exchanges, the other waves evaluate every shape on every wave's
//                        candidate row with pod k added (candidates x shapes lane-jobs, 64 per wave
//                        and round) into the pending rows pnd[wave][shape];
//   after the closing barrier, the wave that owns the winner's slot commits pod k on its row and
//                        copies pnd[that wave][c] to T[c][slot].
// Invariant: after pod k's commit and copy, T[c][s] is the evaluation on the committed state.
// Staging.  No LDS read stands between the exchange's result and pass B, and one between the
// wave's candidate and its statistics: in pod k's exchange window (the idle hook: after the
// statistics barrier, waves 1.. after their refresh jobs, wave 0 ahead of its sweep) every lane
// loads what iteration k+1 reads of its own slot -- T[shape(k+1)][s], T[shape(k+2)][s], the
// static words of pods k+1 and k+2 -- and the wave-uniform record fields (status, creq of pod
// k+1; flags, fit_req of pod k+2) into registers.  After the closing barrier the winner x is
// known: the lane of slot x takes pnd[its wave][shape(k+1)] and pnd[its wave][shape(k+2)] for its
// two table words, exactly what the column copy writes into T; every other staged value is of a
// slot or record pod k's commit does not touch.  Statistics: the lanes select from registers, and
// lane pwv alone reads its candidate's row and static word, as one group of independent loads.
// Every reduction runs where it did, on the same values.  The first iteration of a launch stages
// from the prologue's table.
// Ordering.  A slot's T entries and, between the barriers below, its row are written by the
// wave that owns the slot only, and T is read by that wave only: program order.  The rows are
// read by other waves in the refresh, between the statistics barrier and the closing barrier
// of a pod, and written (the commit) between the closing barrier and the next statistics
// barrier; pnd is written in the first interval and read in the second.  (So the commit is not
// wave 0's, before the closing barrier, as in simple_sync_pw's own: commit = false there.)
// Pod k's commit and column copy are the owner wave's, right behind the winner lane's two pnd
// reads: between pod k's closing barrier and pod k+1's statistics barrier as before, in program
// order before that wave's lane pwv reads its candidate's row (the candidate may be x) and before
// the wave's staging loads of T in window k+1.  Pass B of pod k+1 reads no LDS, so it does not wait
// for them.  (Moving them behind the key reduction of pod k+1 was measured and lost 3 %:
// profiles/r14a_table_staging_ab.txt.)
// Rings.  The prefetch wave stores record and static words of pod k + PD in window k (ring slot
// (k - 1) % RING, whose last readers, pod k-1's refresh and commit, are behind a barrier)
// and only then issues the loads of pod k + PD + 1, which it stores one window later: the HBM
// loads no longer stand in front of that wave's publish.  A ring slot is therefore visible from
// the closing barrier of window (pod - PD) on, as before: window k reads the slots of pods k+1
// and k+2 (the staging; the shape of pod k+2 is read at the top of iteration k), stored in windows
// k-2 and k-1 at the latest and each behind a closing barrier; the slot window k itself writes is
// neither.  Window k0 - 1
// loads pod k0 + PD, the first one the prologue did not.
// FLAT (k_simple_tab_flat): the per-pod reduction and exchange is simple_sync_flat instead of
// simple_sync_pw; the waves' candidates in H.red, the two barriers and everything between them
// are the same, so the ordering above holds for both.
// The shard load / write-back, pending outcome and prefetch below restate simple_schedule's.
// Sharing them as inline helpers changed the code of all five loop kernels (more SGPR spill
// traffic) and cost C1 8.6 %, pct 0 0.9 %, C2 0.3 %: profiles/r10b_loop_pieces_ab.txt.  A change
// to one of these pieces is made in both loops.
// PI (k_simple_tab_pi, k_simple_tab_flat_pi): an image-only batch of the ports-and-images form.
// The static words are k_static_pi's (SWPI_*): raw NodeAffinity in 13 bits, the ImageLocality
// score above it.  ImageLocality is static and has no NormalizeScore, so it is no loop state: pass B
// adds il x weight to the key's total field (pi_key_add's term) and the statistics mask the
// NodeAffinity field; T, the refresh, pnd, the commit, the rings and the ordering above are the
// same.  No pod of such a batch holds a host port (the host checks it), so there is no UsedPorts
// column and no SPort ring in LDS, and the port column in HBM is neither read nor written.
template <bool FLAT, bool PI>
__device__ __forceinline__ void simple_schedule_tab(DevCluster c, const SPod* __restrict__ spods,
                                                    const uint32_t* __restrict__ stat, int k0, int k1, int n_pods,
                                                    int32_t* chosen, PodMeta* meta, int W, int w, int cap,
                                                    unsigned long long* gran, const XPeers& X, unsigned epoch0, int* err,
                                                    unsigned long long* stamps, long long* smem, int n_shapes) {
  constexpr kss_profile prof = default_profile_c();
  constexpr int PD = 3;  // prefetch distance of per-wave mode (simple_schedule): window k stores pod k + PD
  constexpr int PD_TAB = PD + 1;  // ... and loads pod k + PD_TAB, carried one iteration in registers
  static_assert(PD_TAB == RING, "window k stores ring slot (k - 1) % RING: no reader left (see Staging)");
  constexpr int NQ = (int)(sizeof(SPod) / 16);
  const int tid = threadIdx.x, nt = blockDim.x;
  SimpleHdr& H = *reinterpret_cast<SimpleHdr*>(smem);
  const SimpleShard L = shard_view(reinterpret_cast<uint8_t*>(smem) + sizeof(SimpleHdr), cap, 0);
  const ShapeTab TB = shape_tab_view(reinterpret_cast<uint8_t*>(smem), cap, n_shapes);
  const size_t N = (size_t)c.N;
  const int per = (c.N + W - 1) / W;
  const int lo = min(c.N, w * per), hi = min(c.N, lo + per), own = hi - lo;
  if (k1 <= k0) return;
  const int nwave = nt >> 6, lane = tid & 63, wv = tid >> 6;
  const int pwv = (own + nwave - 1) / nwave;  // the wave's node slots (<= PW_LANES)
  const int s = wv * pwv + lane;              // this lane's slot
  const bool mine = lane < pwv && s < own;
  // shard rows, reciprocals, static words and records of pods k0 .. k0 + PD - 1, the shapes -> LDS
  handoff_acquire();
  for (int i = tid; i < own; i += nt) {
    const int n = lo + i;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int64_t A = c.alloc[k * N + n];
      L.r64[k * cap + i] = (double)A;
      L.r64[(3 + k) * cap + i] = (double)ld_ag(&c.requested[k * N + n]);
      L.inv[k * cap + i] = A > 0 ? 1.0 / (double)A : 0.0;
    }
    L.r64[6 * cap + i] = (double)ld_ag(&c.nonzero[n]);
    L.r64[7 * cap + i] = (double)ld_ag(&c.nonzero[N + n]);
    L.r32[i] = ld_ag(&c.pod_count[n]);
    L.r32[cap + i] = c.allowed_pods[n];
    for (int d = 0; d < PD && k0 + d < k1; d++) L.st[((k0 + d) % RING) * cap + i] = ld_ag(&stat[(size_t)d * N + lo + i]);
  }
  for (int i = tid; i < min(k1 - k0, PD) * NQ; i += nt) {
    const int j = k0 + i / NQ;
    reinterpret_cast<uint4*>(L.ring + j % RING)[i % NQ] = reinterpret_cast<const uint4*>(spods + j)[i % NQ];
  }
  for (int j = tid; j < n_shapes; j += nt) {  // record j names the first pod of shape j
    const SPod& r = spods[min(max(spods[j].shape_rep, 0), n_pods - 1)];
    SShape d;
#pragma unroll
    for (int i = 0; i < 3; i++) d.fit_req[i] = r.fit_req[i];
#pragma unroll
    for (int i = 0; i < 2; i++) {
      d.snz[i] = r.snz[i];
      d.sreq[i] = r.sreq[i];
    }
    d.flags = r.flags;
    d.pad = 0;
    uint64_t dw[SSHAPE_WORDS];
    __builtin_memcpy(dw, &d, sizeof(SShape));
#pragma unroll
    for (int i = 0; i < SSHAPE_WORDS; i++) TB.shp[i * n_shapes + j] = dw[i];
  }
  if (tid == 0) H.abort = 0;
  __syncthreads();
  if (mine) {  // the table of the loaded state: every shape on the lane's own slot
    const DynRow r = shard_row(L, s);
    for (int j = 0; j < n_shapes; j++) TB.T[j * TB.ts + s] = shape_pack(dyn_eval_def(shape_get(TB, j), 0u, r));
  }
  __syncthreads();

  KSS_GLOBAL const uint32_t* gstat = gp(stat);
  KSS_GLOBAL const uint4* gspod = gp(reinterpret_cast<const uint4*>(spods));
  KSS_GLOBAL unsigned long long* gstamps = gp(stamps);
  long long R[4] = {0, 0, 0, 0};
  // the outcome of pod pend_k, not yet stored (simple_schedule's deferred outcome: wave 1)
  constexpr int out_tid = 64;
  PodMeta pend{};
  int pend_k = -1;
  auto store_pending = [&]() {
    if (pend_k < 0) return;
    if (chosen) gp(chosen)[pend_k] = pend.chosen;
    if (meta) {
      KSS_GLOBAL PodMeta* mm = gp(meta) + pend_k;
      mm->chosen = pend.chosen;
      mm->n_feasible = pend.n_feasible;
      mm->scored = pend.scored;
      mm->status = pend.status;
      mm->best_total = pend.best_total;
    }
    pend_k = -1;
  };
  int parity = 0;
  unsigned epoch = epoch0;
  const int kb = key_bits(prof, c.N);
  // prefetch lanes as in simple_schedule
  const int pf_w0 = nwave >= 3 ? nwave - 1 : 1;
  const bool pf_wave = __builtin_amdgcn_readfirstlane(tid >> 6) >= pf_w0;
  uint4 pfq = make_uint4(0, 0, 0, 0);
  uint32_t pfw[PF_MAX];
#pragma unroll
  for (int j = 0; j < PF_MAX; j++) pfw[j] = 0;
  const int pf_lane = tid - 64 * pf_w0, pf_n = nt - 64 * pf_w0;
  const int pf_per = (own + pf_n - 1) / pf_n;
  // refresh jobs: job = round * idle lanes + this lane's index among them; job -> (wave v, shape j)
  const int idle_n = 64 * (nwave - 1), jobs = nwave * n_shapes;
  const int job0 = tid - 64;  // (waves 1.. only)
  const int v0 = job0 >= 0 ? job0 / n_shapes : 0, j0 = job0 >= 0 ? job0 % n_shapes : 0;
  // the shapes of pods k+1 and k+2
  int cn = min(max(L.ring[k0 % RING].shape, 0), n_shapes - 1), cnn = 0;
  // the flat exchange: the nodes of the entries this lane holds in the sweep (simple_sync_flat)
  uint32_t er[SXF_LOADS] = {};
  if constexpr (FLAT) {
#pragma unroll
    for (int i = 0; i < SXF_LOADS; i++) er[i] = flat_entry_range(i * 16 + (lane >> 2), per, c.N, W, nwave);
  }
  // the staged operands of iteration kk (pods kk and kk + 1 of shapes ca, cb): see "Staging" above
  uint32_t sa_t = 0, sa_w = 0, sb_t = 0, sb_w = 0;
  int32_t s_status = 0, s_flags = 0;
  double s_creq[3] = {0.0, 0.0, 0.0}, s_fit[3] = {0.0, 0.0, 0.0};
  // Loads only, all independent and none conditional, so that a wave issues them and goes on
  // (wave 0 to its sweep) without waiting: a lane that owns no slot reads slot 0 and a pod outside
  // [k0, k1) whatever its ring slot holds; `mine`, k >= k0 and k + 1 < k1 are applied where the
  // values are used.
  const int ss = mine ? s : 0;
  auto stage = [&](int kk, int ca, int cb) {
    const int ra = (kk + RING) % RING, rb = (kk + 1) % RING;
    sa_t = TB.T[ca * TB.ts + ss];
    sa_w = L.st[ra * cap + ss];
    sb_t = TB.T[cb * TB.ts + ss];
    sb_w = L.st[rb * cap + ss];
    s_status = L.ring[ra].status;
    s_flags = L.ring[rb].flags;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      s_creq[i] = L.ring[ra].creq[i];
      s_fit[i] = L.ring[rb].fit_req[i];
    }
  };
  stage(k0 - 1, 0, cn);  // the first iteration has no earlier window: from the prologue's table
  for (int k = k0 - 1; k < k1; k++) {
    KSS_GLOBAL unsigned long long* sp = (stamps && k >= k0 && k - k0 < KSS_NSTAMP_PODS / 2)
                                            ? gstamps + (size_t)w * 8 * KSS_NSTAMP_PODS + (size_t)(k - k0) * 16
                                            : nullptr;
    if (sp && tid == 0) sp[0] = wall_clock64();
    if (sp && tid == 64) sp[9] = wall_clock64();
    const SPod& pk = L.ring[(k + RING) % RING];
    const int sln = (k + 1) % RING;
    // (pod k+2's record: stored in window k - 1 at the latest, behind its closing barrier)
    if (k + 2 < k1) cnn = min(max(L.ring[(k + 2) % RING].shape, 0), n_shapes - 1);
    // the prefetch wave: record and static words of pod k + PD_TAB are loaded in pod k's exchange
    // window and stored into their ring slots in pod k + 1's
    const bool pf_ld = pf_wave && k + PD_TAB < k1 && own > 0;
    const bool pf_st = pf_wave && k >= k0 && k + PD < k1 && own > 0;  // (what window k - 1 loaded)
    const bool refresh_on = k >= k0 && k + 1 < k1;  // pod k may commit and a pod after it reads the table
    // this iteration's operands leave the staging registers (the window below refills them)
    const uint32_t a_t = sa_t, a_w = sa_w, b_t = sb_t, b_w = sb_w;
    const int32_t k_status = s_status, n_flags = s_flags;
    const double k_creq[3] = {s_creq[0], s_creq[1], s_creq[2]}, n_fit[3] = {s_fit[0], s_fit[1], s_fit[2]};
    // pass B: pod k's table word and static word (staged), arithmetic on registers
    const long long nf = R[1];
    const int max_tt = (int)R[2], max_na = (int)R[3];
    const bool scored = nf > 1;
    const bool keys = k >= k0 && k_status == 0 && nf > 0;
    const float rtt = __builtin_amdgcn_rcpf((float)max(max_tt, 1));
    const float rna = __builtin_amdgcn_rcpf((float)max(max_na, 1));
    long long best = 0;
    {
      const int a_na = PI ? (int)((uint32_t)sw_na(a_w) & SWPI_NA_MAX) : sw_na(a_w);
      const SVal e{sw_code(a_w), sw_tt(a_w), a_na, (int)((a_t >> 8) & 0xFFu), (int)(a_t & 0xFFu)};
      long long key = simple_key(prof, e, scored, max_tt, rtt, max_na, rna, (uint32_t)(c.node_base + lo + s));
      if constexpr (PI) {  // ImageLocality: its raw score is final; unsigned (il = 100 sets bit 31 of the word)
        const uint32_t il = a_w >> SWPI_IL_SHIFT;
        key += scored ? (long long)((unsigned long long)(il * (uint32_t)prof.weight[KSS_S_IMAGE_LOCALITY]) << 32) : 0ll;
      }
      best = (keys && mine && e.f == 0 && (a_t & ST_FITS)) ? key : 0;
    }
    if (sp && tid == 0) sp[1] = wall_clock64();
    best = wave_max_key(best, kb, c.node_base);
    if (sp && tid == 0) sp[2] = wall_clock64();
    const int cand = best ? (int)(0xFFFFFFFFu - (uint32_t)(unsigned long long)best) - c.node_base - lo : -1;
    // statistics of pod k+1: H0 from the staged table word; H1 on the wave's candidate with pod k
    // added, whose row and static word lane pwv alone reads (one group of independent loads)
    uint32_t u[6] = {0, 0, 0, 0, 0, 0};
    if (k + 1 < k1) {
      const bool extra = lane == pwv && cand >= 0;
      bool ok = mine && (b_t & ST_FITS) != 0;
      uint32_t wd = b_w;
      if (extra) {  // fitsRequest of pod k+1 on the row after AssumePod(pod k): the verdict alone
        const int ns = cand;
        wd = L.st[sln * cap + ns];
        const int32_t pods = L.r32[ns], allowed = L.r32[cap + ns];
        double al[3], rq[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          al[i] = L.r64[i * cap + ns];
          rq[i] = L.r64[(3 + i) * cap + ns];
        }
        bool bad = (int64_t)pods + 2 > (int64_t)allowed;
        bool sh = false;
#pragma unroll
        for (int i = 0; i < 3; i++) sh |= n_fit[i] > al[i] - (rq[i] + k_creq[i]);
        bad |= !(n_flags & SP_ALLZERO) & sh;
        ok = !bad;
      }
      ok &= sw_code(wd) == 0;
      const bool c0 = ok && !extra, c1 = ok && (extra || s != cand);
      const uint32_t tt = (uint32_t)sw_tt(wd), na = PI ? ((uint32_t)sw_na(wd) & SWPI_NA_MAX) : (uint32_t)sw_na(wd);
      u[0] = c0 ? 1u : 0u;
      u[1] = c0 ? tt : 0u;
      u[2] = c0 ? na : 0u;
      u[3] = c1 ? 1u : 0u;
      u[4] = c1 ? tt : 0u;
      u[5] = c1 ? na : 0u;
    }
    if (sp && tid == 0) sp[3] = wall_clock64();
    auto idle = [&]() {
      // the refresh: waves 1.. (wave 0 exchanges), the waves' candidates from the reduction rows
      // of this pod (parity not yet flipped), each on its row with pod k added
      if (refresh_on && keys && wv > 0) {
        for (int job = job0, rd = 0; job < jobs; job += idle_n, rd++) {
          const int v = rd == 0 ? v0 : job / n_shapes, j = rd == 0 ? j0 : job % n_shapes;
          const long long kv = H.red[parity][v][0];
          if (kv == 0) continue;
          const int cs = (int)(0xFFFFFFFFu - (uint32_t)(unsigned long long)kv) - c.node_base - lo;
          DynRow r = shard_row(L, cs);
          add_commit(r, pk);
          TB.pnd[v * KSS_MAX_SHAPES + j] = shape_pack(dyn_eval_def(shape_get(TB, j), 0u, r));
        }
        if (sp && (tid == 64 || tid == 128)) sp[11 + (tid >> 6)] = wall_clock64();  // waves 1, 2: refresh done
      }
      // the operands of pod k + 1's iteration (every wave; wave 0 issues them ahead of its sweep)
      stage(k + 1, cn, cnn);
      if (pf_st) {  // the record and static words loaded one window ago -> their ring slots
        reinterpret_cast<uint4*>(L.ring + (k + PD) % RING)[min(pf_lane, NQ - 1)] = pfq;
#pragma unroll
        for (int j = 0; j < PF_MAX; j++)
          if (j < pf_per) L.st[((k + PD) % RING) * cap + min(j * pf_n + pf_lane, own - 1)] = pfw[j];
      }
      if (pf_ld) {  // ... and the next ones, behind this wave's publish
        KSS_GLOBAL const uint4& src = gspod[(size_t)(k + PD_TAB) * NQ + min(pf_lane, NQ - 1)];
        pfq = make_uint4(src.x, src.y, src.z, src.w);
#pragma unroll
        for (int j = 0; j < PF_MAX; j++)
          if (j < pf_per) pfw[j] = ld_ag(&gstat[(size_t)(k + PD_TAB - k0) * N + lo + min(j * pf_n + pf_lane, own - 1)]);
      }
      if (tid == out_tid) store_pending();  // the previous pod's outcome
    };
    bool synced;
    if constexpr (FLAT)
      synced = simple_sync_flat(H, parity, best, u, W, w, ++epoch, gran, X, err, c.node_base, kb, er, R, sp, idle);
    else
      synced = simple_sync_pw(H, parity, best, u, W, w, ++epoch, gran, X, err, per, c.node_base, lo, own, pk, false, L, kb,
                              R, sp, idle);
    if (!synced) return;
    if (sp && tid == 0) sp[5] = wall_clock64();
    if (k >= k0) {
      const long long K = R[0];
      const int x = K ? (int)(0xFFFFFFFFu - (uint32_t)(unsigned long long)K) - c.node_base : -1;
      // the wave that owns the winner's slot: the winner's lane takes the pending values of pods
      // k+1 and k+2 (what its next pass B waits for), then AssumePod on the row and the pending row
      // into the table -- LDS traffic that pass B, register arithmetic, no longer waits behind
      if (x >= lo && x < hi && (x - lo) / max(pwv, 1) == wv) {
        if (refresh_on && s == x - lo) {
          sa_t = TB.pnd[wv * KSS_MAX_SHAPES + cn];
          sb_t = TB.pnd[wv * KSS_MAX_SHAPES + cnn];
        }
        simple_commit_lanes(L, pk, x - lo, lane);
        if (refresh_on && lane < n_shapes) TB.T[lane * TB.ts + (x - lo)] = TB.pnd[wv * KSS_MAX_SHAPES + lane];
      }
      if (w == X.w_off && tid == out_tid) {
        pend.chosen = K ? x + c.node_base : -1;
        pend.n_feasible = (int)nf;
        pend.scored = (K && scored) ? 1 : 0;
        pend.status = k_status != 0 ? (k_status == KSS_PF_ERROR ? 3 : 2) : (nf == 0 ? 1 : 0);
        pend.best_total = pend.scored ? (int64_t)((unsigned long long)K >> 32) : 0;
        pend_k = k;
      }
    }
    cn = cnn;
    if (sp && tid == 0) sp[6] = wall_clock64();
  }
  if (tid == out_tid) store_pending();  // the last pod's outcome
  // node state back to HBM
  __syncthreads();
  for (int i = tid; i < own; i += nt) {
    const int n = lo + i;
#pragma unroll
    for (int r = 0; r < 3; r++) st_ag(&c.requested[(size_t)r * N + n], (int64_t)L.r64[(3 + r) * cap + i]);
    st_ag(&c.nonzero[n], (int64_t)L.r64[6 * cap + i]);
    st_ag(&c.nonzero[N + n], (int64_t)L.r64[7 * cap + i]);
    st_ag(&c.pod_count[n], L.r32[i]);
  }
  handoff_release();
}

// The class / term count part of AssumePod for pods [k0, k1) of a k_simple batch, from
// their chosen nodes (one lane per pod; counts commute, so the order is immaterial).
__device__ __forceinline__ void simple_counts(const DevCluster& c, const SPod* __restrict__ spods,
                                              const int32_t* __restrict__ ints, const int32_t* __restrict__ chosen,
                                              int k) {
  const int x = chosen[k] - c.node_base;
  if (x < 0 || x >= c.N) return;
  const SPod& q = spods[k];
  const size_t N = (size_t)c.N;
  if (q.cls >= 0) atomicAdd(&c.class_count[(size_t)q.cls * N + x], 1);
  for (int i = 0; i < q.own_len; i++) atomicAdd(&c.term_count[(size_t)ints[q.own_off + i] * N + x], 1);
}

}  // namespace kss
