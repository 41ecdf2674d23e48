/*
 * nffacl.h — C-ABI of libnffacl, the MI355X-native replacement for nff-go's
 * L3/L4 ACL hot path (packet/acl.go + the header parsing of packet/packet.go).
 *
 * Every entry point is plain C: pointers, sizes and integer status codes; no
 * HIP, torch or C++ types cross this boundary (a HIP stream is passed as
 * `void*`).  A Go cgo package, a Python ctypes binding and the C++ host mirror
 * (nff-go_amd/host/nffgo.hpp) all bind exactly these symbols.
 *
 * Reference interfaces replaced (paths relative to aregm/nff-go):
 *   nffacl_rules_load_text      <- packet.GetL3ACLFromTextTable   packet/acl.go:148-178
 *   nffacl_rules_parse_text     <- same parser, from a memory buffer (acl.go:156-177)
 *   nffacl_rules_load_json      <- packet.GetL3ACLFromJSON        packet/acl.go:121-134
 *   nffacl_rules_from_arrays    <- L3Rules{ip4: ..., ip6: ...} literals the reference
 *                                  tests build directly (acl_internal_test.go:588-593)
 *   nffacl_rules_get4/get6      <- the unexported ip4/ip6 slices read by the reference
 *                                  parse tests (acl_internal_test.go:392, 420)
 *   nffacl_classify_device      <- (*Packet).L3ACLPort / L3ACLPermit  acl.go:495-506,
 *                                  l3ACL acl.go:522-565, l4ACL acl.go:508-520,
 *                                  ParseAllKnownL3 packet.go:353-363,
 *                                  ParseL4ForIPv4/6 packet.go:278-285 — over a batch of
 *                                  packets resident in HBM
 *   nffacl_classify_frames_device  same, over packed variable-length frames (IMIX)
 *   nffacl_extract_keys_frames_device  the same parse over packed frames, into 16-byte keys
 *   nffacl_extract_keys_encap_frames_device <- the decapsulation that precedes it for tunnelled
 *                                  traffic (vlan.go, mpls.go, gre.go, gtp.go:132-140): keys of the
 *                                  inner headers, the frames left as they are
 *   nffacl_route_gather_frames_device <- the per-output packet slices of segmentProcess
 *                                  (flow/flow.go:1462-1486) as packed frames with
 *                                  descriptors, gathered through a route's index lists
 *   nffacl_route_gather_decap_frames_device <- the same with RemoveVLANTag / RemoveMPLS /
 *                                  DecapsulateIPv4GTP (packet.go:789-798) done on the way
 *   nffacl_route_gather_encap_frames_device <- the same with AddVLANTag / AddMPLS /
 *                                  EncapsulateIPv4GTP (packet.go:758-771), the next hop's MACs
 *                                  and the TTL decrement done on the way
 *   nffacl_checksum_frames_device <- CalculateIPv4Checksum, CalculateIPv{4,6}{TCP,UDP,ICMP}Checksum
 *                                  (packet/checksum.go:186-345) over packed frames, each
 *                                  compared with the field the frame carries
 *   nffacl_classify_host        <- the VectorSeparateFunction body the reference runs per
 *                                  burst (flow/flow.go:131, 1487-1520;
 *                                  test/stability/testSingleWorkingFF/testSingleWorkingFF.go:538-546)
 *                                  — host slots in, verdicts out, PCIe staging inside
 *   nffacl_engine_swap_rules    <- the atomic *L3Rules pointer swap user code performs
 *                                  on rule reload (examples/tutorial/step08.go:33-44)
 *   nffacl_batcher_*            <- the per-burst VectorSeparateFunction calls of every
 *                                  flow-function clone (flow/flow.go:131, 1487-1520),
 *                                  aggregated across threads into shared GPU batches
 *   nffacl_l2rules_load_text    <- packet.GetL2ACLFromTextTable   packet/acl.go:88-117
 *   nffacl_l2rules_load_json    <- packet.GetL2ACLFromJSON        packet/acl.go:70-84
 *   nffacl_l2_classify_device   <- (*Packet).L2ACLPort / L2ACLPermit  acl.go:462-491
 *                                  (l2ACL acl.go:478-491) over a batch in HBM
 *
 * Verdict semantics (bit-exact with acl.go):
 *   port  = OutputNumber of the FIRST rule (file order, per address family) that
 *           matches, 0 if none or the packet is neither IPv4 nor IPv6;
 *   permit = port > 0.
 * Packet bytes past the end of the slot/frame read as 0 (the reference reads
 * whatever mbuf memory follows; the slot convention pins that to zero).
 *
 * Status codes: 0 on success, negative on error.  The rule-parser codes are the
 * negated nff-go common.ErrorCode values (common/error.go:18-50) so a cgo shim
 * can rebuild the exact NFError{Code} the reference returns.
 *
 * Threading: rules objects are immutable after creation and may be shared by
 * any number of threads.  An engine may be used concurrently from several host
 * threads (each on its own stream); nffacl_engine_swap_rules may run
 * concurrently with classification and takes effect for launches issued after
 * it returns.
 */
#ifndef NFFACL_H
#define NFFACL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFFACL_ABI_VERSION 7

/* Only the entry points below are exported from libnffacl.so (built with
 * -fvisibility=hidden). */
#if defined(__GNUC__)
#define NFFACL_API __attribute__((visibility("default")))
#else
#define NFFACL_API
#endif

/* ---- status codes ------------------------------------------------------ */
enum nffacl_status {
    NFFACL_OK = 0,
    /* negated common.ErrorCode (common/error.go:18-50) */
    NFFACL_ERR_PARSE_RULE_JSON = -11,      /* ParseRuleJSONErr */
    NFFACL_ERR_FILE = -12,                 /* FileErr */
    NFFACL_ERR_PARSE_RULE = -13,           /* ParseRuleErr ("Incomplete 5-tuple") */
    NFFACL_ERR_INCORRECT_ARG_IN_RULES = -14, /* IncorrectArgInRules */
    NFFACL_ERR_INCORRECT_RULE = -15,       /* IncorrectRule (bad OutputNumber) */
    /* engine / device errors (no reference counterpart) */
    NFFACL_ERR_INVALID_ARG = -100,
    NFFACL_ERR_NOMEM = -101,
    NFFACL_ERR_HIP = -102,
    NFFACL_ERR_NO_DEVICE = -103,
    NFFACL_ERR_UNSUPPORTED = -104,
    NFFACL_ERR_TIMEOUT = -105    /* a bounded wait ran out (the work may still complete) */
};

/* ---- rule records (internal representation of acl.go:423-449) --------- */

/* l4Rules, acl.go:423-431 */
typedef struct nffacl_l4 {
    uint8_t id;            /* L4 protocol number (types.TCPNumber ...) */
    uint8_t id_mask;       /* 0 = ANY, 0xff = exact */
    uint8_t valid;         /* ports constrained (IPv4 rules skip the port test when 0) */
    uint8_t reserved;      /* must be 0 */
    uint16_t src_port_min; /* host-order port numbers */
    uint16_t src_port_max;
    uint16_t dst_port_min;
    uint16_t dst_port_max;
} nffacl_l4; /* 12 bytes */

/* l3Rules4, acl.go:433-440.  Addresses and masks are types.IPv4Address values:
 * the little-endian uint32 of the four wire bytes (types/ipv4.go:13-28), so
 * 127.0.0.1 is 0x0100007f exactly as in the reference. */
typedef struct nffacl_rule4 {
    uint32_t output_number; /* Go `uint`; the parsers bound it to 32 bits */
    uint32_t src_addr;
    uint32_t dst_addr;
    uint32_t src_mask;
    uint32_t dst_mask;
    nffacl_l4 l4;
} nffacl_rule4; /* 32 bytes */

/* l3Rules6, acl.go:442-449.  Wire byte order. */
typedef struct nffacl_rule6 {
    uint32_t output_number;
    uint8_t src_addr[16];
    uint8_t dst_addr[16];
    uint8_t src_mask[16];
    uint8_t dst_mask[16];
    nffacl_l4 l4;
} nffacl_rule6; /* 80 bytes */

typedef struct nffacl_rules nffacl_rules;
typedef struct nffacl_engine nffacl_engine;

/* ---- rules ------------------------------------------------------------- */

/* GetL3ACLFromTextTable (acl.go:148).  On error *out is NULL and `err`
 * (if non-NULL) receives the message.  The reference additionally hands back a
 * partially filled *L3Rules next to the error (acl.go:177); no caller uses it. */
NFFACL_API int nffacl_rules_load_text(const char *path, nffacl_rules **out, char *err, size_t errlen);
/* Same grammar, parsing `len` bytes of an in-memory file image. */
NFFACL_API int nffacl_rules_parse_text(const char *text, size_t len, nffacl_rules **out, char *err,
                            size_t errlen);
/* GetL3ACLFromJSON (acl.go:121). */
NFFACL_API int nffacl_rules_load_json(const char *path, nffacl_rules **out, char *err, size_t errlen);
NFFACL_API int nffacl_rules_parse_json(const char *text, size_t len, nffacl_rules **out, char *err,
                            size_t errlen);
/* Build a rule set from already-parsed records, as the reference tests build
 * L3Rules literals (arrays are copied; either pointer may be NULL when its
 * count is 0). */
NFFACL_API int nffacl_rules_from_arrays(const nffacl_rule4 *r4, size_t n4, const nffacl_rule6 *r6,
                             size_t n6, nffacl_rules **out);
NFFACL_API void nffacl_rules_free(nffacl_rules *rules);
NFFACL_API int nffacl_rules_counts(const nffacl_rules *rules, size_t *n4, size_t *n6);
NFFACL_API int nffacl_rules_get4(const nffacl_rules *rules, size_t i, nffacl_rule4 *out);
NFFACL_API int nffacl_rules_get6(const nffacl_rules *rules, size_t i, nffacl_rule6 *out);

/* Compile `rules` for HIP device `hip_device` and upload the table now; the
 * calls that take a rule set per call (nffacl_service_classify,
 * nffacl_batcher_submit_rules) otherwise do this on first use.  The table
 * belongs to the rule set: nffacl_rules_free retires it (stream-ordered
 * behind the work that used it).  This is what makes the reference's rule
 * reload — build a new *L3Rules, swap the pointer (examples/tutorial/
 * step08.go:38-44) — work unchanged: every call classifies against exactly
 * the rule set it was given.  A rule set must outlive the calls using it. */
NFFACL_API int nffacl_rules_prepare(const nffacl_rules *rules, int hip_device);

/* The HIP device the calling thread (a flow-function clone) should use, or
 * NFFACL_ERR_NO_DEVICE: ABI 6 spreads the clones of a NUMA node over ALL of
 * that node's GPUs — the device is nffacl_pick_device() of the thread's CPU
 * (its rank among its node's CPUs, modulo the node's device count; every
 * device when none is on the node).  Stable per thread: its first call
 * decides.  nff-go pins every clone to a core (flow/scheduler.go:283-289,
 * internal/low/low.go:654-666), so the clones of a 2-socket, 8-GPU node land
 * on all 8 GPUs (ABI 5 gave every clone the node's first GPU).  Replaces the
 * binding's former hard-wired GPU 0. */
NFFACL_API int nffacl_local_device(void);

/* The device map behind nffacl_local_device, on any topology: CPU `cpu`
 * (cpu_node[c] = NUMA node of CPU c, -1 unknown; n_cpus entries) gets device
 * local[rank % |local|], where local = the devices d with dev_node[d] equal
 * to the CPU's node (all devices when none) and rank = the number of CPUs
 * below `cpu` on its node.  NFFACL_ERR_INVALID_ARG on bad arguments. */
NFFACL_API int nffacl_pick_device(int cpu, const int *cpu_node, int n_cpus, const int *dev_node, int n_devs);

/* The NUMA node of a HIP device's PCIe attachment (>= 0), or a negative
 * status (NFFACL_ERR_INVALID_ARG, NFFACL_ERR_NO_DEVICE; NFFACL_ERR_HIP when
 * the platform does not report one).  One-packet calls through
 * nffacl_service_classify are fastest from threads on this node (the
 * mailboxes are allocated there): pin the flow-function clones (DPDK lcores)
 * to it.  32 callers on the device's node: 5.8-5.9 Mpps; on the other
 * socket: 3.9-4.4. */
NFFACL_API int nffacl_device_numa_node(int hip_device);

/* ---- engine ------------------------------------------------------------ */

/* Matching strategy compiled into the device table. */
enum nffacl_algo {
    NFFACL_ALGO_AUTO = 0,   /* library picks (indexed when the rule set allows) */
    NFFACL_ALGO_LINEAR = 1, /* wave-uniform first-match scan (acl.go's loop order) */
    NFFACL_ALGO_INDEXED = 2, /* host-compiled interval index + ordered candidate lists */
    NFFACL_ALGO_HYBRID = 3   /* the same index for tables larger than LDS: bucket
                                directories in LDS, compact 16-byte candidates and
                                per-rule records in HBM (CIDR rule sets; AUTO picks
                                it when the INDEXED table outgrows LDS) */
};

/* Compile `rules` for HIP device `hip_device` and upload the table. */
NFFACL_API int nffacl_engine_create(int hip_device, const nffacl_rules *rules, nffacl_engine **out);
NFFACL_API int nffacl_engine_create_ex(int hip_device, const nffacl_rules *rules, int algo,
                            nffacl_engine **out);
/* Compile + upload a new table, then atomically make it the active one.
 * Launches issued before the call keep using the previous table. */
NFFACL_API int nffacl_engine_swap_rules(nffacl_engine *eng, const nffacl_rules *rules);
NFFACL_API void nffacl_engine_destroy(nffacl_engine *eng);
/* Algorithm actually compiled into the active table (NFFACL_ALGO_LINEAR/INDEXED/HYBRID). */
NFFACL_API int nffacl_engine_algo(const nffacl_engine *eng);
/* Bytes of the active device table (rule records + index), for reporting. */
NFFACL_API int nffacl_engine_table_bytes(const nffacl_engine *eng, uint64_t *bytes);

/* The kernel the active table's launches over dense 64-byte slots take
 * (inspection and tests; ABI 7). */
enum nffacl_walk {
    NFFACL_WALK_LINEAR = 0,          /* wave-uniform rule scan (k_linear_slots) */
    NFFACL_WALK_INDEXED_GLOBAL = 1,  /* per-lane candidate lists, table in global memory */
    NFFACL_WALK_INDEXED_LDS = 2,     /* per-lane candidate lists, table staged in LDS */
    NFFACL_WALK_HYBRID_LANE = 3,     /* LDS directories, per-lane walks of HBM entries */
    NFFACL_WALK_FLAT = 4,            /* flat candidate walk, directories in global memory */
    NFFACL_WALK_FLAT_LDS = 5,        /* flat candidate walk, directories in LDS (classify_flat) */
    NFFACL_WALK_FLAT_LDS_GENERIC = 6,/* the same over generalized (compacted) slots */
    NFFACL_WALK_FLAT_LDS_PIPELINED = 7 /* pipelined family-split walk (classify_flat_pipe) */
};
typedef struct nffacl_kernel_info {
    int32_t walk;        /* enum nffacl_walk */
    uint32_t slots;      /* key slots the kernel walks (its NS) */
    uint32_t rounds;     /* flat walks: entry-load rounds per window (2 or 4); else 0 */
    uint32_t block;      /* threads per workgroup */
    uint32_t per_cu;     /* workgroups launched per CU */
    int32_t load_mode;   /* packet load mode at stride 64 (engine.hip) */
    uint32_t pulled;     /* 1: waves pull their batches at run time (BatchSource) */
    uint32_t reserved;
    uint64_t lds_bytes;  /* dynamic LDS per workgroup */
} nffacl_kernel_info;
NFFACL_API int nffacl_engine_kernel_info(nffacl_engine *eng, nffacl_kernel_info *out);

/* Host-side compilation of a rule set into the device table blob, without a
 * device (tooling / inspection; the engine runs the same compiler).  Call with
 * blob == NULL to learn info->blob_dwords, then again with a buffer of at
 * least that many dwords. */
typedef struct nffacl_dim_info {
    uint32_t kind;       /* key: 0 src4, 1 dst4, 2 src6 (top 32 bits), 3 dst6, 4 sport, 5 dport */
    uint32_t shift;      /* bucket = key >> shift (1-D); see kind2 */
    uint32_t n_buckets;  /* radix buckets */
    uint32_t off_dir;    /* dword offset of dir[n_buckets + 1] (bucket bounds, in entries) */
    uint32_t off_entries;/* dword offset of the bucket entries (inline rules, ascending per bucket) */
    uint32_t n_rules;    /* rules indexed by this key */
    uint32_t max_list;   /* longest bucket list */
    uint32_t off_dir16;  /* 0, or (two-level directory) dword offset of u16 offsets dir16[n_buckets + 1];
                            then off_dir holds u32 group bases and dir[t] = base[t >> 6] + dir16[t] */
    uint64_t n_entries;  /* bucket entries (with replication) */
    uint32_t kind2;      /* 6 = none (1-D slot); else a second key (kinds as above): the slot is a
                            2-D grid, bucket = (key >> shift) << bits2 | key2 >> shift2 */
    uint32_t shift2, bits2;
    uint32_t dir8;       /* 1: off_dir16 holds u8 offsets dir8[n_buckets + 1] and off_dir the u32 bases
                            of 16-bucket groups: dir[t] = base[t >> 4] + dir8[t] */
} nffacl_dim_info;

#define NFFACL_MAX_SLOTS 8

typedef struct nffacl_family_info {
    uint32_t n_rec;        /* live rules of the family */
    uint32_t off_rec;      /* LINEAR: dword offset of the rule records (8 dwords IPv4, 20 IPv6);
                              HYBRID flat forms: of the output array (one u32 per rule) */
    uint32_t entry_dwords; /* INDEXED / lane form: dwords per entry (8 IPv4, 20 IPv6);
                              HYBRID flat forms: 6 IPv4, 12 IPv6 (exact entries) */
    uint32_t off_resid, n_resid; /* INDEXED: entries scanned linearly (no selective key) */
    nffacl_dim_info dims[NFFACL_MAX_SLOTS]; /* INDEXED: [dst addr, src addr, dst port, src port];
                                               HYBRID global-directory form: any 1-D / 2-D keys */
    uint32_t n_slots;            /* slots in use (dims[0, n_slots)) */
    uint32_t off_ent_base;       /* HYBRID flat forms: dword offset of the family's first entry
                                    (directory values are entry numbers counted from it) */
} nffacl_family_info;

typedef struct nffacl_table_info {
    int32_t algo;        /* NFFACL_ALGO_LINEAR, _INDEXED or _HYBRID */
    uint32_t lds_dwords; /* HYBRID: blob[0, lds_dwords) = the directories staged in LDS */
    uint64_t blob_dwords;
    nffacl_family_info fam[2]; /* [0] IPv4, [1] IPv6 */
    uint32_t off_params; /* HYBRID flat-LDS positional forms: the slot parameter block in the LDS image (0: none) */
    uint32_t reserved;
} nffacl_table_info;

NFFACL_API int nffacl_table_compile(const nffacl_rules *rules, int algo, uint32_t *blob,
                                    uint64_t cap_dwords, nffacl_table_info *info);

/* ---- classification ------------------------------------------------------ */

/* Parse flags (the *_ex entry points).  0 = the reference's l3ACL exactly. */
enum nffacl_parse_flags {
    /* Parse L3 with ParseAllKnownL3CheckVLAN (packet/vlan.go:104-117) instead
     * of ParseAllKnownL3: one 802.1Q tag (EtherType 0x8100) moves the L3
     * header 4 bytes and the tag's EtherType selects IPv4/IPv6.  The
     * reference's L3ACLPermit never does this (a tagged frame gets 0); the
     * flag serves pipelines that composed the VLAN-aware parse themselves. */
    NFFACL_PARSE_VLAN = 1u
};

/* Device-resident dense slots: packet i occupies d_slots[i*stride, (i+1)*stride)
 * with its frame starting at byte 0 (the Ether header) and zero padding after
 * the frame.  stride % 16 == 0, stride >= 64, d_slots 16-byte aligned.
 * d_port[i]  <- L3ACLPort (may be NULL)
 * d_permit_bits[i/64] bit i%64 <- L3ACLPermit (may be NULL; ceil(n/64) words;
 *   bits past n in the last word are 0).
 * Asynchronous on `stream` (hipStream_t, NULL = default stream).  Launches
 * of one engine on one stream run in stream order; the large-table kernels
 * hand out their batches through per-stream counters of the engine, so a
 * launch captured into a graph must not be replayed concurrently with
 * launches of the same engine on the stream it was captured from (or set
 * NFFACL_TUNE_DYN=0 before creating the engine). */
NFFACL_API int nffacl_classify_device(nffacl_engine *eng, const uint8_t *d_slots, uint32_t stride,
                           uint64_t n, uint32_t *d_port, uint64_t *d_permit_bits,
                           void *stream);

/* Device-resident packed frames (IMIX): frame i starts at d_frames + (desc[i] >> 16)
 * and is (desc[i] & 0xffff) bytes long; bytes past its length read as 0.
 * Frame starts must be 16-byte aligned (mbuf data rooms are cache-line aligned). */
NFFACL_API int nffacl_classify_frames_device(nffacl_engine *eng, const uint8_t *d_frames,
                                  const uint64_t *d_desc, uint64_t n, uint32_t *d_port,
                                  uint64_t *d_permit_bits, void *stream);

/* The same with parse flags (enum nffacl_parse_flags). */
NFFACL_API int nffacl_classify_device_ex(nffacl_engine *eng, const uint8_t *d_slots, uint32_t stride,
                                         uint64_t n, uint32_t *d_port, uint64_t *d_permit_bits,
                                         void *stream, uint32_t flags);
NFFACL_API int nffacl_classify_frames_device_ex(nffacl_engine *eng, const uint8_t *d_frames,
                                                const uint64_t *d_desc, uint64_t n, uint32_t *d_port,
                                                uint64_t *d_permit_bits, void *stream, uint32_t flags);

/* Host slots in, host verdicts out: pinned staging + async H2D / kernel / D2H,
 * double-buffered across chunks.  Synchronous.  h_port / h_permit may be NULL
 * (h_permit gets one byte per packet, 0 or 1). */
NFFACL_API int nffacl_classify_host(nffacl_engine *eng, const uint8_t *h_slots, uint32_t stride,
                         uint64_t n, uint32_t *h_port, uint8_t *h_permit);
NFFACL_API int nffacl_classify_host_ex(nffacl_engine *eng, const uint8_t *h_slots, uint32_t stride,
                                       uint64_t n, uint32_t *h_port, uint8_t *h_permit, uint32_t flags);

/* ---- compact 5-tuple keys (additive to ABI 7) -----------------------------
 *
 * The walk needs only what the header parse extracts: family, protocol, two
 * ports, two addresses.  A key holds exactly those fields of one packet — 16
 * bytes for IPv4 instead of a 64-byte slot — so a flow-function clone that
 * fills keys moves a quarter of the bytes over PCIe / xGMI / HBM, and a batch
 * parsed once can be classified against several rule sets or again after
 * nffacl_engine_swap_rules without touching packet bytes.  Reference
 * interfaces stood for:
 *   nffacl_extract_keys_device / _host <- ParseAllKnownL3 (packet.go:353-363;
 *       ParseAllKnownL3CheckVLAN, vlan.go:104-117, under NFFACL_PARSE_VLAN) +
 *       ParseL4ForIPv4/6 (packet.go:278-285) and the field reads of l3ACL /
 *       l4ACL (acl.go:508-565), done once per packet
 *   nffacl_classify_keys_device <- (*Packet).L3ACLPort / L3ACLPermit
 *       (acl.go:495-506) over the extracted fields of a batch in HBM
 *   nffacl_classify_keys_host   <- the VectorSeparateFunction body
 *       (flow/flow.go:131, 1487-1520), keys in, verdicts out
 * A key is what the parse yields for its packet: ports come from wherever IHL
 * puts them, bytes past the frame read as 0, ports are read for ICMP too, a
 * VLAN tag is honoured only under NFFACL_PARSE_VLAN. */
typedef struct nffacl_key {   /* 16 bytes; arrays 16-byte aligned */
    uint32_t a;      /* family 4: src, a types.IPv4Address as in nffacl_rule4.src_addr
                        family 6: index of this packet's nffacl_key6 record */
    uint32_t b;      /* family 4: dst; family 6: 0 */
    uint32_t ports;  /* sport | dport << 16, host-order numbers */
    uint32_t meta;   /* bits 0-7 L4 protocol, bits 8-15 family (0 = neither, 4, 6), rest 0 */
} nffacl_key;
typedef struct nffacl_key6 { uint8_t src[16]; uint8_t dst[16]; } nffacl_key6; /* wire order, 32 bytes */

/* d_port / d_permit_bits / stream as nffacl_classify_device, for n keys in
 * HBM (d_keys and d_key6 16-byte aligned; d_key6 may be NULL when n_key6 is
 * 0).  A key of family 0, of an unknown family, or of family 6 with an index
 * >= n_key6 gets verdict 0, and nothing outside the two arrays is read.
 * Serves every table an engine can hold.  The key kernels take static
 * batches (no per-stream counters): launches may be captured and replayed
 * freely. */
NFFACL_API int nffacl_classify_keys_device(nffacl_engine *eng, const nffacl_key *d_keys,
                                           const nffacl_key6 *d_key6, uint32_t n_key6, uint64_t n,
                                           uint32_t *d_port, uint64_t *d_permit_bits, void *stream);
/* d_keys[i] <- the key of slot i (slots as nffacl_classify_device, flags as
 * nffacl_parse_flags); an IPv6 packet's record goes to d_key6[i] and its key
 * carries index i, so d_key6 holds n records and only IPv6 packets write
 * theirs (classify with n_key6 = n).  n < 2^32.  Asynchronous on `stream`. */
NFFACL_API int nffacl_extract_keys_device(const uint8_t *d_slots, uint32_t stride, uint64_t n, uint32_t flags,
                                          nffacl_key *d_keys, nffacl_key6 *d_key6, void *stream);
/* d_keys[i] <- the key of frame i (frames as nffacl_classify_frames_device, flags as
 * nffacl_parse_flags): the parse of ParseAllKnownL3 (packet.go:353-363) over
 * packed frames, bytes past a frame's length read as 0.  key6 placement and
 * limits as nffacl_extract_keys_device. */
NFFACL_API int nffacl_extract_keys_frames_device(const uint8_t *d_frames, const uint64_t *d_desc, uint64_t n,
                                                 uint32_t flags, nffacl_key *d_keys, nffacl_key6 *d_key6,
                                                 void *stream);
/* The same on the CPU, for the clones: frames[i] points at packet i's Ether
 * header, lens[i] is its readable bytes (bytes past it read as 0).  IPv6
 * records are packed densely into key6[0, *n_key6) in arrival order;
 * NFFACL_ERR_INVALID_ARG (nothing promised about the outputs) when more than
 * key6_cap are needed.  key6 may be NULL when key6_cap is 0. */
NFFACL_API int nffacl_extract_keys_host(const uint8_t *const *frames, const uint32_t *lens, uint64_t n,
                                        uint32_t flags, nffacl_key *keys, nffacl_key6 *key6, uint64_t key6_cap,
                                        uint64_t *n_key6);
/* Host keys in, host verdicts out (outputs as nffacl_classify_host), through
 * the engine's chunked pinned staging: pinned 16-byte aligned key arrays are
 * read by the kernel where they lie, pageable ones are staged.  Synchronous. */
NFFACL_API int nffacl_classify_keys_host(nffacl_engine *eng, const nffacl_key *h_keys, const nffacl_key6 *h_key6,
                                         uint32_t n_key6, uint64_t n, uint32_t *h_port, uint8_t *h_permit);

/* ---- keys of encapsulated frames (additive to ABI 7) ----------------------
 *
 * The traffic the reference decapsulates on the CPU before it classifies the
 * inner 5-tuple (vlan.go, mpls.go: ParseL3CheckMPLS / RemoveMPLS, gre.go,
 * gtp.go: DecapsulateIPv4GTP), resolved at extraction time instead: the key is
 * that of the inner header, the frame is not rewritten, and every key call
 * downstream works unchanged.
 *
 * Layers are resolved outermost-in, each only if its flag is set and it is
 * present; resolution stops at the first layer that is not enabled.  The
 * cursor is the offset of the L3 header and starts at 14:
 *  1. VLAN: while the EtherType at cursor-2 is 0x8100 or 0x88A8 and fewer than
 *     2 tags were taken, cursor += 4.
 *  2. MPLS: if that EtherType is 0x8847, labels of 4 bytes are skipped through
 *     the first with the S bit; more than 8 is malformed.  The reference leaves
 *     label -> protocol to the caller; here the usual rule holds: the version
 *     nibble of the next byte gives the family (4, 6, anything else family 0).
 *  3. One tunnel level, if the L3 header at the cursor is IPv4 (any IHL >= 5)
 *     or a fixed 40-byte IPv6 header (no extension headers) that carries
 *     - GRE: protocol 47, version 0; 4 bytes plus 4 for each of the C, K and S
 *       bits; NextProto 0x0800 / 0x86DD is the inner family, else family 0;
 *     - GTP-U: UDP to port 2152, GTPv1, PT 1, message type 255; 8 bytes, 12
 *       with any of E / S / PN; with E the extension headers are walked
 *       (length in 4-octet units, 0 is malformed, next type in the last octet,
 *       at most 4); the family is the version nibble.  For the frames
 *       DecapsulateIPv4GTP handles this is its IPv4MinLen + UDPLen + GTPMinLen.
 * The key is what nffacl_extract_keys_frames_device(flags = 0) gives for the
 * frame with bytes [14, cursor) removed and the EtherType set to the resolved
 * family: ports from wherever the inner IHL puts them, ports for ICMP, bytes
 * past the length as 0.  A frame that matches nothing enabled gets its plain
 * key (cursor 14, whatever its length), so encap = 0 is the plain call and
 * mixed traffic needs no sorting.  A malformed frame — a cap exceeded, a GTP
 * extension of length 0, or shims resolved up to or past the frame's end
 * (cursor > 14 and cursor >= length) — gets the all-zero key (family 0,
 * verdict 0).  Bytes past the length read as 0 during resolution too: a
 * frame cut before a field that identifies a layer does not carry that layer. */
enum nffacl_encap_flags {
    NFFACL_ENCAP_VLAN = 1u,   /* up to 2 stacked tags, TPID 0x8100 or 0x88A8, 4 bytes each (vlan.go:66-76) */
    NFFACL_ENCAP_MPLS = 2u,   /* EtherType 0x8847: labels of 4 bytes up to the bottom-of-stack bit
                                 (mpls.go:38-41, 65-74), at most 8 */
    NFFACL_ENCAP_GRE  = 4u,   /* IPv4 or IPv6 outer, protocol 47, GRE version 0 (gre.go:13-16) */
    NFFACL_ENCAP_GTPU = 8u    /* IPv4 or IPv6 outer, UDP dport 2152, GTPv1, PT = 1, message type 255
                                 (gtp.go:19-28, 62-64, 132-140) */
};
/* d_keys[i] <- the inner key of frame i under `encap` (nffacl_encap_flags).
 * Frames, descriptors, alignment, key6 placement (d_key6[i], index i in the
 * key), n < 2^32 and asynchrony as nffacl_extract_keys_frames_device; nothing
 * outside a frame's 16-byte chunks is read.  d_inner_off (may be NULL; 2-byte
 * aligned) gets the cursor of frame i — 14 for an unencapsulated frame — or
 * 0xFFFF for a malformed one.  NFFACL_ERR_INVALID_ARG for unknown encap bits,
 * NULL or misaligned buffers, n >= 2^32.  No atomics, no allocation: launches
 * may be captured and replayed freely. */
NFFACL_API int nffacl_extract_keys_encap_frames_device(const uint8_t *d_frames, const uint64_t *d_desc, uint64_t n,
                                                       uint32_t encap, nffacl_key *d_keys, nffacl_key6 *d_key6,
                                                       uint16_t *d_inner_off, void *stream);

/* ---- checksums of packed frames (additive to ABI 7) -----------------------
 *
 * What packet/checksum.go computes per packet on the CPU, and what the NIC's
 * RX offload checks on the reference's own path, for a batch that stays in
 * HBM: the IPv4 header sum and the TCP / UDP / ICMP sum of every frame, each
 * compared with the field the frame carries.  Frames are not written.
 *
 * Per frame: L is its length; c is the cursor, 14 if d_inner_off is NULL,
 * else d_inner_off[i] as nffacl_extract_keys_encap_frames_device writes it.
 * Bytes are on the wire, "words" are big-endian 16-bit words, fold is
 * reduceChecksum (checksum.go:179-184).
 *
 * Family.  c odd (0xFFFF is), c < 14 or c >= L: the all-zero record.  c == 14:
 * EtherType 0x0800 is IPv4, 0x86DD IPv6, anything else the all-zero record,
 * and the version nibble at byte c must agree or the record is all zero.
 * c > 14: the version nibble at byte c decides (4, 6, else all zero), the rule
 * of the encap call below MPLS and GTP-U.
 *
 * IPv4 header.  H = 4 * IHL.  IHL < 5, c + 20 > L or c + H > L: the record is
 * LENGTH only.  Under NFFACL_CK_IP4, ip = ~fold(words of [c, c + H) with the
 * checksum field as 0) — options count, which CalculateIPv4Checksum ignores —
 * and IP4_DONE is set; IP4_BAD if the stored field differs, 0x0000 and 0xFFFF
 * comparing equal.
 *
 * IPv4 L4, under NFFACL_CK_L4.  T is TotalLength.  T < H or c + T > L: LENGTH.
 * Otherwise, any of bits 0x3FFF of the word at c + 6 (MF, fragment offset):
 * FRAGMENT.  Otherwise the protocol must be 6, 17 or 1, or nothing is
 * computed.  The span is [c + H, c + T), m = T - H bytes; Ethernet padding past
 * T is not part of it.  m below 20 (TCP) or 8 (UDP, ICMP), or a UDP DgramLen
 * other than m: LENGTH.  Otherwise l4 = ~fold(words of the span, an odd last
 * byte padded with 0 on the right, its checksum field (offset 16 TCP, 6 UDP,
 * 2 ICMP) as 0, plus the pseudo-header: the source and destination words, the
 * protocol and m; none for ICMP), for UDP a result of 0 becomes 0xFFFF, and
 * L4_DONE is set.  A UDP field stored as 0 sets L4_ABSENT and never L4_BAD;
 * otherwise L4_BAD as for the header.
 *
 * IPv6 L4, under NFFACL_CK_L4 (an IPv6 frame's record is all zero without
 * it).  The header is the fixed 40 bytes: c + 40 > L or c + 40 + PayloadLen > L
 * is LENGTH.  The next header must be 6, 17 or 58 directly (an extension
 * header means no L4 sum, as elsewhere in this library).  The span is
 * [c + 40, c + 40 + PayloadLen), minimum lengths and DgramLen as for IPv4; the
 * pseudo-header is the 16 address words, PayloadLen and the next header, for
 * all three protocols.  A UDP field stored as 0 is L4_BAD.
 *
 * ip and l4 are host-order numbers, as the reference's functions return them:
 * for well-formed IHL-5 packets they are what CalculateIPv4Checksum,
 * CalculateIPv{4,6}{TCP,UDP}Checksum and CalculateIPv{4,6}ICMPChecksum return.
 * Divergences: IPv4 options count, in the header sum and in where L4 starts
 * (the reference subtracts IPv4MinLen whatever the IHL); lengths are checked
 * against the frame (the reference sums whatever memory follows). */
enum nffacl_cksum_what { NFFACL_CK_IP4 = 1u, NFFACL_CK_L4 = 2u };
enum nffacl_cksum_status {
    NFFACL_CK_IP4_DONE = 1u,  NFFACL_CK_IP4_BAD = 2u,
    NFFACL_CK_L4_DONE  = 4u,  NFFACL_CK_L4_BAD  = 8u,
    NFFACL_CK_L4_ABSENT = 16u, /* UDP over IPv4 sent without a checksum (field 0): computed, never BAD */
    NFFACL_CK_FRAGMENT  = 32u, /* IPv4 MF set or fragment offset != 0: no L4 sum */
    NFFACL_CK_LENGTH    = 64u  /* a header or a length field claims bytes the frame does not have,
                                  or is below its minimum: what depends on it is not computed */
};
typedef struct nffacl_cksum { uint16_t ip; uint16_t l4; uint32_t status; } nffacl_cksum; /* 8 bytes, arrays 8-byte aligned */
/* d_sums[i] (may be NULL) <- frame i's record, every frame's written, zero
 * where nothing applies; bit i of d_bad_bits (may be NULL; ceil(n / 64) words,
 * the last word's spare bits 0) <- IP4_BAD | L4_BAD of it.  `what` is a
 * non-empty set of nffacl_cksum_what.  Frames, descriptors, alignment,
 * n < 2^32 and asynchrony as nffacl_extract_keys_frames_device; d_inner_off
 * is 2-byte aligned; nothing outside a frame's 16-byte chunks is read.  No
 * global atomics, no allocation, no scratch: launches may be captured and
 * replayed freely.  NFFACL_ERR_INVALID_ARG, with no launch, for unknown `what`
 * bits or what == 0, both outputs NULL, NULL or misaligned buffers,
 * n >= 2^32. */
NFFACL_API int nffacl_checksum_frames_device(const uint8_t *d_frames, const uint64_t *d_desc, uint64_t n,
                                             const uint16_t *d_inner_off, uint32_t what, nffacl_cksum *d_sums,
                                             uint64_t *d_bad_bits, void *stream);
/* Pure, no device: *tiles >= 1, a workgroup's tile is ceil(n / tiles) frames. */
NFFACL_API int nffacl_checksum_frames_plan(uint64_t n, uint64_t *tiles);

/* ---- burst aggregator (host ingest) ----------------
 *
 * Many threads (the reference's flow-function clones, each with a burst of
 * <= 32 packets) submit bursts; the library copies each packet's first
 * `stride` bytes into a shared pinned slot ring and ships the open batch as
 * soon as fewer than two batches are on the GPU — so batches grow while the
 * GPU is busy, up to `max_batch` packets — and every submitter of that batch
 * sleeps until its verdicts are back.  A batch whose first burst has waited
 * `max_delay_us` ships whatever else is in flight.  Thread-safe: any number of
 * concurrent submitters per batcher.  Every ticket must be waited for exactly
 * once (its batch buffer is reused only then).  Tickets not yet waited for
 * keep their batches' buffers busy: a batch ships at the latest when its first
 * burst is max_delay_us old, so a caller that submits without waiting can hold
 * as few as one burst per buffer.  When every buffer is busy, submit waits for
 * one to free (back-pressure) at most 1 s and then returns NFFACL_ERR_TIMEOUT
 * without a ticket (the bursts held are the caller's own to collect).
 * Each batch carries its own status: a failed launch fails the bursts of that
 * batch only.  A batch classifies against one table — the engine's active
 * table, or the rule set a burst was submitted with (nffacl_batcher_*_rules):
 * bursts for different rule sets never share a batch.
 */
typedef struct nffacl_batcher nffacl_batcher;

typedef struct nffacl_ticket {
    uint64_t seq;
    uint32_t buf, off, n, reserved;  /* reserved: the burst's number in its batch */
} nffacl_ticket;

typedef struct nffacl_batcher_stats {
    uint64_t batches;  /* GPU launches */
    uint64_t packets;  /* packets classified */
    uint64_t bursts;   /* submit calls */
    uint64_t timeouts; /* batches shipped before max_batch filled */
} nffacl_batcher_stats;

/* stride: slot bytes per packet (multiple of 16, >= 64; 80 keeps IPv4 with IHL
 * 15 exact); max_batch: packets per GPU launch (>= 64); nbuf: batch buffers in
 * rotation (>= 2).  The engine must outlive the batcher. */
NFFACL_API int nffacl_batcher_create(nffacl_engine *eng, uint32_t stride, uint32_t max_batch,
                                     uint32_t max_delay_us, uint32_t nbuf, nffacl_batcher **out);
/* A batcher of HIP device `hip_device` with no engine: every burst names its
 * rule set (nffacl_batcher_submit_rules / _classify_rules), the binding's
 * shape for the reference's per-call *L3Rules (examples/tutorial/step08.go:
 * 33-44: clones load the current pointer, a reload goroutine stores a new
 * one). */
NFFACL_API int nffacl_batcher_create_device(int hip_device, uint32_t stride, uint32_t max_batch,
                                            uint32_t max_delay_us, uint32_t nbuf, nffacl_batcher **out);
/* Queue a burst: frames[i] points at packet i's Ether header, lens[i] its
 * bytes (NULL lens: `stride` bytes each; bytes past a length read as 0).
 * n <= max_batch.  Returns without waiting; *ticket identifies the burst.
 * Engine batchers only (the engine's active table at launch). */
NFFACL_API int nffacl_batcher_submit(nffacl_batcher *b, const uint8_t *const *frames, const uint32_t *lens,
                                     uint32_t n, nffacl_ticket *ticket);
/* The same against `rules` (its own table on the batcher's device, compiled
 * on first use; nffacl_rules_prepare).  `rules` must outlive the wait. */
NFFACL_API int nffacl_batcher_submit_rules(nffacl_batcher *b, const nffacl_rules *rules,
                                           const uint8_t *const *frames, const uint32_t *lens, uint32_t n,
                                           nffacl_ticket *ticket);
/* Block until the burst's batch is classified; ports[i] <- L3ACLPort of packet
 * i.  Returns the batch's status; a second wait on a ticket is rejected. */
NFFACL_API int nffacl_batcher_wait(nffacl_batcher *b, const nffacl_ticket *ticket, uint32_t *ports);
/* The same, giving up after timeout_us: NFFACL_ERR_TIMEOUT means the batch is
 * not done yet (shipped or not) — no verdict, and the ticket stays valid: wait
 * on it again. */
NFFACL_API int nffacl_batcher_wait_timeout(nffacl_batcher *b, const nffacl_ticket *ticket, uint32_t *ports,
                                           uint64_t timeout_us);
/* submit + wait: the body of a VectorSeparateFunction. */
NFFACL_API int nffacl_batcher_classify(nffacl_batcher *b, const uint8_t *const *frames, const uint32_t *lens,
                                       uint32_t n, uint32_t *ports);
NFFACL_API int nffacl_batcher_classify_rules(nffacl_batcher *b, const nffacl_rules *rules,
                                             const uint8_t *const *frames, const uint32_t *lens, uint32_t n,
                                             uint32_t *ports);
/* Ship the currently open batch now (do not wait for max_batch / max_delay_us). */
NFFACL_API int nffacl_batcher_flush(nffacl_batcher *b);
NFFACL_API int nffacl_batcher_get_stats(nffacl_batcher *b, nffacl_batcher_stats *out);
/* Ships queued bursts, waits for the batches in flight, then frees; no
 * submit/wait may be running. */
NFFACL_API void nffacl_batcher_destroy(nffacl_batcher *b);

/* ---- scalar calls: persistent GPU consumer ------------------------------
 *
 * (*Packet).L3ACLPort / L3ACLPermit (acl.go:495-506) called ONE packet at a
 * time, the shape of every SetSeparator / SetSplitter user function
 * (flow/flow.go:128, 1795-1797; examples/firewall/firewall.go:54-57;
 * examples/tutorial/step08.go:33-35).  A service keeps one small kernel
 * resident on its GPU that polls per-thread mailboxes in pinned host memory:
 * a call writes its packet's first 80 bytes into the calling thread's
 * mailbox and waits until the kernel has written the verdict back — no
 * kernel launch, no driver call per packet.  A caller spins; once the callers
 * outnumber the CPUs the process may use (affinity, cgroup quota) it first
 * sleeps through most of the round trip (a nap adapted per mailbox), so that
 * waiting callers leave the CPUs to posting ones.  The kernel exits after
 * `idle_us` without calls (and every 100 ms) and is re-armed by the next
 * call.  Thread-safe; one service per GPU serves every thread.
 */
typedef struct nffacl_service nffacl_service;

typedef struct nffacl_service_stats {
    uint64_t launches;  /* consumer kernel launches (re-arms) */
    uint64_t requests;  /* calls answered */
    uint64_t timeouts;  /* calls that returned NFFACL_ERR_TIMEOUT */
    uint64_t running;   /* 1 while the consumer kernel is resident */
    uint64_t table_oob; /* 1 if a table walk ever indexed outside its table (read as 0 instead
                           of faulting; a compiler/upload bug — the tests require 0) */
    /* where the time goes, summed over the consumer's completed launches: */
    uint64_t polls;     /* mailbox polls (one PCIe read of every hot mailbox each) */
    double poll_ns;     /* mean poll duration, load issue to data */
    uint64_t groups;    /* request groups classified (one table per group) */
    double group_ns;    /* mean time to classify + answer a group */
    uint64_t answered;  /* requests answered by the consumer (packets) */
    uint64_t retries;   /* requests re-posted after a first timeout (see the failure policy below) */
    uint64_t torn;      /* polls that read a request while its caller was still writing it (re-read) */
} nffacl_service_stats;

/* mailboxes: a multiple of 64 (one consumer wave per 8; 0 = 128), one per
 * calling thread (threads beyond that share mailboxes under a lock);
 * idle_us: consumer lifetime without calls (0 = 2000). */
NFFACL_API int nffacl_service_create(int hip_device, uint32_t mailboxes, uint32_t idle_us, nffacl_service **out);
/* A burst service (ABI 5): the VectorSeparateFunction shape — every call
 * carries a clone's whole burst of up to 32 packets (flow/flow.go:131,
 * 1487-1520: segmentProcess hands the separator one burst at a time and
 * waits for its answers).  One mailbox per calling thread (mailboxes 1..1024,
 * 0 = 64), one consumer wave per mailbox; a request is one rule set. */
NFFACL_API int nffacl_service_create_burst(int hip_device, uint32_t mailboxes, uint32_t idle_us,
                                           nffacl_service **out);
/* L3ACLPort of one packet: frame = its Ether header, len its bytes (bytes past
 * len, and past 80, read as 0 — the batcher's 80-byte slot); flags:
 * enum nffacl_parse_flags.  *port <- the verdict (permit = port > 0).  Blocks
 * about one PCIe round trip.  On a burst service: a burst of one.
 *
 * Failure policy (the reference's verdict path never errors, acl.go:522-565;
 * a caller must not crash the flow function it runs in): a call with no answer
 * after 1 s (NFFACL_TUNE_SVC_TIMEOUT_US) re-posts its request once and re-arms
 * the consumer (stats.retries); with no answer after another 1 s it withdraws
 * the request (the consumer answers a withdrawn request without reading any
 * table, so the rules may be freed at once), sets the verdict(s) to 0 —
 * reject, the value l3ACL gives a packet that matches no rule — and returns
 * NFFACL_ERR_TIMEOUT (stats.timeouts).  Bindings use the verdict and count the
 * event instead of failing the flow function.  Later calls
 * are served normally once the consumer runs again. */
NFFACL_API int nffacl_service_classify(nffacl_service *svc, const nffacl_rules *rules, const uint8_t *frame,
                                       uint32_t len, uint32_t flags, uint32_t *port);
/* L3ACLPort of a burst (burst services only): frames[i] / lens[i] as above
 * (lens NULL: 80 bytes each), n <= 32; ports[i] <- the verdict of packet i.
 * One PCIe round trip for the whole burst; failure policy as above. */
NFFACL_API int nffacl_service_classify_burst(nffacl_service *svc, const nffacl_rules *rules,
                                             const uint8_t *const *frames, const uint32_t *lens, uint32_t n,
                                             uint32_t flags, uint32_t *ports);
/* paused != 0: stop the resident consumer and launch none until resumed (GPU
 * maintenance; calls meanwhile follow the failure policy); 0: resume. */
NFFACL_API int nffacl_service_pause(nffacl_service *svc, int paused);
NFFACL_API int nffacl_service_get_stats(nffacl_service *svc, nffacl_service_stats *out);
/* Stops the consumer and frees; no call may be running. */
NFFACL_API void nffacl_service_destroy(nffacl_service *svc);

/* ---- L2 ACL (packet/acl.go:68-117, 356-383, 413-421, 457-491) ----------- */

/* l2Rules, acl.go:413-421.  MAC addresses in wire order; `id` is the EtherType
 * as a host-order number (types.IPV4Number = 0x0800 ...), compared with the
 * frame's big-endian EtherType under `id_mask` (0 = ANY, 0xffff = exact). */
typedef struct nffacl_l2_rule {
    uint32_t output_number;
    uint8_t daddr_not_any; /* 1: daddr must equal Ether.DAddr (frame bytes 0..5) */
    uint8_t saddr_not_any; /* 1: saddr must equal Ether.SAddr (frame bytes 6..11) */
    uint8_t daddr[6];
    uint8_t saddr[6];
    uint16_t id_mask;
    uint16_t id;
    uint16_t reserved; /* must be 0 */
} nffacl_l2_rule; /* 24 bytes */

typedef struct nffacl_l2rules nffacl_l2rules;
typedef struct nffacl_l2engine nffacl_l2engine;

/* GetL2ACLFromTextTable (acl.go:88): "SrcMAC DstMAC ID [Rule]" per line. */
NFFACL_API int nffacl_l2rules_load_text(const char *path, nffacl_l2rules **out, char *err, size_t errlen);
NFFACL_API int nffacl_l2rules_parse_text(const char *text, size_t len, nffacl_l2rules **out, char *err,
                                         size_t errlen);
/* GetL2ACLFromJSON (acl.go:70): {"L2Rules": [{"Source", "Destination", "ID", "Rule"}]}. */
NFFACL_API int nffacl_l2rules_load_json(const char *path, nffacl_l2rules **out, char *err, size_t errlen);
NFFACL_API int nffacl_l2rules_parse_json(const char *text, size_t len, nffacl_l2rules **out, char *err,
                                         size_t errlen);
/* L2Rules{eth: ...} literal (acl_internal_test.go:1186-1193); copied. */
NFFACL_API int nffacl_l2rules_from_array(const nffacl_l2_rule *r, size_t n, nffacl_l2rules **out);
NFFACL_API void nffacl_l2rules_free(nffacl_l2rules *rules);
NFFACL_API int nffacl_l2rules_count(const nffacl_l2rules *rules, size_t *n);
NFFACL_API int nffacl_l2rules_get(const nffacl_l2rules *rules, size_t i, nffacl_l2_rule *out);

/* algo: NFFACL_ALGO_LINEAR (file-order scan) or NFFACL_ALGO_INDEXED (one hashed
 * probe per rule shape; AUTO picks it when the rules use <= 8 distinct
 * MAC/EtherType mask shapes, which every parsed rule file does). */
NFFACL_API int nffacl_l2_engine_create(int hip_device, const nffacl_l2rules *rules, nffacl_l2engine **out);
NFFACL_API int nffacl_l2_engine_create_ex(int hip_device, const nffacl_l2rules *rules, int algo,
                                          nffacl_l2engine **out);
NFFACL_API int nffacl_l2_engine_algo(const nffacl_l2engine *eng);
NFFACL_API int nffacl_l2_engine_swap_rules(nffacl_l2engine *eng, const nffacl_l2rules *rules);
NFFACL_API void nffacl_l2_engine_destroy(nffacl_l2engine *eng);

/* L2ACLPort / L2ACLPermit over device-resident slots / packed frames; same
 * buffer conventions as nffacl_classify_device / _frames_device (only frame
 * bytes 0..13 are read; bytes past a frame's length read as 0). */
NFFACL_API int nffacl_l2_classify_device(nffacl_l2engine *eng, const uint8_t *d_slots, uint32_t stride,
                                         uint64_t n, uint32_t *d_port, uint64_t *d_permit_bits,
                                         void *stream);
NFFACL_API int nffacl_l2_classify_frames_device(nffacl_l2engine *eng, const uint8_t *d_frames,
                                                const uint64_t *d_desc, uint64_t n, uint32_t *d_port,
                                                uint64_t *d_permit_bits, void *stream);
/* Host slots in, host verdicts out (synchronous; staging inside, sized to the
 * request).  h_port / h_permit (one byte per packet) may be NULL. */
NFFACL_API int nffacl_l2_classify_host(nffacl_l2engine *eng, const uint8_t *h_slots, uint32_t stride,
                                       uint64_t n, uint32_t *h_port, uint8_t *h_permit);

/* ---- device group: one process, several GPUs (ABI 6) -------------------
 * The reference's multi-core deployment is ONE process whose core-pinned
 * clones share one *L3Rules (flow/scheduler.go:283-289, packet/acl.go:
 * 495-506); a group lets such a host spread one batch over several GPUs
 * without a process per GPU.  nffacl_group_create opens one RCCL
 * communicator per device (ncclCommInitAll), compiles `rules` once on the
 * host, uploads the table to hip_devices[0] (the root) and ncclBroadcasts
 * it to the others over xGMI.  The group owns its tables (the rule set may
 * be freed afterwards); a rule reload is a new group.  Devices must be
 * distinct.  NFFACL_ERR_NO_DEVICE without HIP devices; NFFACL_ERR_HIP with
 * the last error "RCCL not available: ..." when librccl cannot be loaded —
 * RCCL is opened here (dlopen), so nothing else in the library needs it.
 * Every RCCL call and device switch is checked; a failure inside a group
 * call closes the group and returns NFFACL_ERR_HIP.  (Groups of more than
 * one device have run on no multi-GPU node yet: their scatter / gather
 * parity is unverified on hardware) */
typedef struct nffacl_group nffacl_group;
NFFACL_API int nffacl_group_create(const int *hip_devices, int n, const nffacl_rules *rules, nffacl_group **out);
NFFACL_API int nffacl_group_size(const nffacl_group *g);
/* L3ACLPort / L3ACLPermit of n packets resident on the ROOT device (slots as
 * nffacl_classify_device; d_port / d_permit_bits on the root too, either may
 * be NULL but not both): 64-aligned shards go to the group's devices by
 * ncclSend/ncclRecv (the root keeps the first), every device classifies its
 * shard, and the verdicts (ports, permit words) come back by ncclSend/
 * ncclRecv into the root's arrays.  Enqueued on `stream` (a root-device
 * hipStream_t; NULL = default) and the group's own per-device streams:
 * returns at once; the verdicts are complete when `stream` is.  Calls on one
 * group are serialised (they share its communicators). */
NFFACL_API int nffacl_group_classify_device(nffacl_group *g, const uint8_t *d_slots, uint32_t stride, uint64_t n,
                                            uint32_t *d_port, uint64_t *d_permit_bits, void *stream);
NFFACL_API void nffacl_group_destroy(nffacl_group *g);
/* The group's shard plan (pure; ABI 7): shard i of n packets over n_devices
 * devices is [*off, *off + *len) — shards of ceil(ceil(n / N) / 64) * 64
 * packets in device order, the last ones shorter or empty, *off always a
 * multiple of 64 (so the shard's permit words start at *off / 64 and no
 * word straddles two devices).  NFFACL_ERR_INVALID_ARG for N outside 1..64,
 * i outside 0..N-1, n > 2^48 or NULL outputs. */
NFFACL_API int nffacl_group_shard(uint64_t n, int n_devices, int i, uint64_t *off, uint64_t *len);

/* ---- routing: per-output index lists of a classified batch ---------------
 * SetSeparator / SetSplitter do not return verdicts, they route: the scalar
 * loop of segmentProcess appends every packet of a burst to
 * OutputMbufs[answer] in arrival order and enqueues one slice per output flow
 * (flow/flow.go:1462-1486; the vector form through asm.GenerateMask,
 * flow.go:1505-1517) — a stable partition of the burst by answer.  A router
 * computes that partition for a verdict vector resident in HBM (the d_port of
 * the classify calls above), entirely on the device.  Additive to ABI 7. */
enum nffacl_route_mode {
    NFFACL_ROUTE_SEPARATE = 0, /* n_out = 2, output = (port != 0): separate, flow.go:1795-1797 —
                                  the rejected flow is output 0, the accepted flow output 1 */
    NFFACL_ROUTE_SPLIT = 1     /* output = port, n_out = the splitter's flowNumber, 1..255
                                  (makeSplitter(..., uint8(flowNumber)), flow.go:1161).  A port >=
                                  n_out indexes next[] out of range in the reference (the Go
                                  runtime panics); here such packets form one extra out-of-range
                                  segment after the last output, and are counted. */
};
typedef struct nffacl_router nffacl_router;
/* A router for batches of up to max_n (<= 2^31) packets on `hip_device`.  It
 * owns its scratch (per-tile counts, sized by max_n here; launches allocate
 * nothing, so they can be captured into a graph) and serves launches in
 * stream order on one stream at a time: one router per stream. */
NFFACL_API int nffacl_router_create(int hip_device, uint32_t mode, uint32_t n_out, uint64_t max_n,
                                    nffacl_router **out);
/* d_index[n] <- a permutation of 0..n-1: the indices of output 0's packets in
 * ascending (arrival) order, then output 1's, ..., the out-of-range segment
 * last — OutputMbufs[0], [1], ... of flow.go:1462-1486 laid end to end.
 * d_offsets[n_out + 2]: [o] = start of output o's segment, [n_out] = start of
 * the out-of-range segment, [n_out + 1] = n.  n = 0 writes only the offsets.
 * Asynchronous on `stream` (three kernel launches; no workgroup waits on
 * another).  NFFACL_ERR_INVALID_ARG for NULL pointers or n > max_n. */
NFFACL_API int nffacl_route_device(nffacl_router *r, const uint32_t *d_port, uint64_t n, uint32_t *d_index,
                                   uint32_t *d_offsets, void *stream);
/* d_out slot j <- slot d_index[j] of d_slots, j < m (the packets of an output
 * slice made dense, e.g. for a D2H of the permitted packets only; slots as
 * nffacl_classify_device: stride % 16 == 0, stride >= 64, both buffers 16-byte
 * aligned, else NFFACL_ERR_INVALID_ARG). */
NFFACL_API int nffacl_route_gather_device(const uint8_t *d_slots, uint32_t stride, const uint32_t *d_index,
                                          uint64_t m, uint8_t *d_out, void *stream);
/* The router's plan (pure, no device): the tiles n packets are cut into and
 * the scratch bytes a router of max_n = n holds, tiles * (n_out + 1) * 4.
 * NFFACL_ERR_INVALID_ARG for n > 2^31, n_out outside 1..255 or NULL outputs. */
NFFACL_API int nffacl_route_plan(uint64_t n, uint32_t n_out, uint64_t *tiles, uint64_t *scratch_bytes);
/* The per-output packet lists of segmentProcess (flow/flow.go:1462-1486) for
 * packed frames.  Output frame j (j < m) <- frame d_index[j] of (d_frames,
 * d_desc[0..n)), packed:
 *   room(len)     = len rounded up to `align` (a power of two, 16..4096)
 *   off_j         = sum_{k<j} room(len_k)                       (64-bit)
 *   d_out_desc[j] = off_j << 16 | len_j
 *   d_out[off_j, off_j+len_j) = the frame's bytes; [off_j+len_j, off_j+room) = 0
 *   *d_out_bytes  = sum of all rooms (the bytes the packed batch needs)
 * so (d_out, d_out_desc) is a frames batch for nffacl_classify_frames_device.
 * Called with the whole d_index of a route it yields every output's frames
 * back to back (d_offsets cuts d_out_desc into the outputs); with d_index +
 * offsets[o] and that output's count, one output.
 * d_index[j] >= n counts as an empty frame (len 0; nothing is read for it).
 * Nothing at or past d_out + out_cap is written (out_cap % 16 == 0).  16-byte
 * chunks wholly below it are written, and d_out_desc and *d_out_bytes are
 * complete either way, so the caller sees from *d_out_bytes > out_cap that the
 * buffer was short.
 * Source frames as nffacl_classify_frames_device: 16-byte aligned starts
 * (d_frames and d_out 16-byte aligned).  A 16-byte chunk is read only if it
 * starts inside its frame.  Bytes past len in the last chunk are not copied
 * (zeroed).  d_index may repeat an index.
 * m <= the router's max_n.  m = 0 writes only *d_out_bytes = 0.  Asynchronous
 * on `stream` (three kernel launches); launches allocate nothing; recorded on
 * the router's event like nffacl_route_device, and sharing its one-stream
 * rule.  NFFACL_ERR_INVALID_ARG for a bad align or out_cap, NULL or misaligned
 * buffers, m > max_n. */
NFFACL_API int nffacl_route_gather_frames_device(nffacl_router *r, const uint8_t *d_frames, const uint64_t *d_desc,
                                                 uint64_t n, const uint32_t *d_index, uint64_t m, uint32_t align,
                                                 uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_desc,
                                                 uint64_t *d_out_bytes, void *stream);
/* The same gather, decapsulating on the way (additive to ABI 7): what the
 * reference's users do between classifying the inner header and the enqueue —
 * RemoveVLANTag, RemoveMPLS, DecapsulateIPv4GTP (gtp.go:132-140), i.e.
 * DecapsulateHead(EtherLen, length) (packet.go:789-798), which drops the bytes
 * [14, 14 + length) and keeps the Ethernet header in front of the payload.
 * d_inner_off[0..n) and d_keys[0..n) are what
 * nffacl_extract_keys_encap_frames_device wrote for (d_frames, d_desc); both
 * are required (NULL, d_inner_off not 2-byte or d_keys not 16-byte aligned:
 * NFFACL_ERR_INVALID_ARG).  Of a key only the `meta` dword is read.
 * For source frame i = d_index[j] < n of length L and cursor c = d_inner_off[i]:
 *   strip   s = c - 14 if 14 < c < L and (c - 14) % 4 == 0, else s = 0: an
 *           unencapsulated frame (14), a malformed one (0xFFFF) and any value
 *           the extraction does not produce are copied whole, and a bad cursor
 *           never makes the call read outside the frame
 *   length  L' = L - s; d_out_desc[j] = off_j << 16 | L'; the room is L'
 *           rounded up to `align`, pads zeroed
 *   bytes   [0, 12) the source's; [12, 14) the EtherType E, big-endian;
 *           [14, L') source bytes [14 + s, L)
 *   E       s == 0: the source's bytes 12-13 (the frame is bit-identical to
 *           what nffacl_route_gather_frames_device writes); else by the family
 *           in d_keys[i].meta: 4 -> 0x0800, 6 -> 0x86DD, any other -> source
 *           bytes [c - 2, c).  Those are the inner EtherType behind VLAN tags
 *           and the NextProto of an option-less GRE header; behind an MPLS
 *           stack or a GRE header with options they are NOT an EtherType (the
 *           end of the last label, of the last option).  Such frames have
 *           family 0 and get verdict 0 whatever E says.
 * For every frame the extraction did not mark malformed,
 * nffacl_extract_keys_frames_device(flags = 0) on (d_out, d_out_desc) gives
 * the key nffacl_extract_keys_encap_frames_device gave for the source frame.
 * Everything else — packing, align, out_cap, *d_out_bytes, the empty frame for
 * d_index[j] >= n, repeated indices, m <= max_n, m = 0, three launches, no
 * allocation, the router's event and one-stream rule, alignment of d_frames
 * and d_out, a 16-byte source chunk read only if it starts inside its frame —
 * is as nffacl_route_gather_frames_device; the scratch is the same
 * (nffacl_route_frames_plan). */
NFFACL_API int nffacl_route_gather_decap_frames_device(nffacl_router *r, const uint8_t *d_frames,
                                                       const uint64_t *d_desc, uint64_t n,
                                                       const uint16_t *d_inner_off, const nffacl_key *d_keys,
                                                       const uint32_t *d_index, uint64_t m, uint32_t align,
                                                       uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_desc,
                                                       uint64_t *d_out_bytes, void *stream);
/* The same gather, rewriting for the next hop on the way (additive to ABI 7):
 * what a forwarder does between the route lookup and the enqueue — the next
 * hop's Ethernet addresses, the TTL decrement of examples/decrementTTL.go:27-40,
 * and AddVLANTag (vlan.go:119-131), AddMPLS (mpls.go:81-91) or
 * EncapsulateIPv4GTP (gtp.go:117-130) with the outer header fill of
 * examples/gtpu.go:62-95, i.e. EncapsulateHead(EtherLen, length)
 * (packet.go:758-771), which opens `length` bytes behind the Ethernet header.
 * One nffacl_adj record describes one next hop's rewrite: */
enum nffacl_adj_flags {
    NFFACL_ADJ_MACS        = 1u,  /* output bytes [0,12) <- dmac, smac */
    NFFACL_ADJ_TTL         = 2u,  /* decrement the source frame's IPv4 TTL / IPv6 hop limit (below) */
    NFFACL_ADJ_INNER_ETYPE = 4u,  /* shim bytes [s-2, s) <- the source's bytes 12-13 (a tag's inner type, GRE NextProto); s >= 4 */
    NFFACL_ADJ_IP4_LEN     = 8u,  /* the shim opens with a 20-byte IPv4 header: TotalLength, HdrChecksum filled; s >= 20 */
    NFFACL_ADJ_UDP_LEN     = 16u, /* + UDP behind it: DgramLen filled; needs IP4_LEN, s >= 28 */
    NFFACL_ADJ_GTP_LEN     = 32u  /* + GTPv1 behind that: MessageLength filled; needs UDP_LEN, s >= 36 */
};
typedef struct nffacl_adj {       /* 64 bytes, arrays 16-byte aligned: one next hop's rewrite */
    uint8_t  dmac[6], smac[6];
    uint16_t ether_type;          /* host-order number; 0 = keep the source's */
    uint8_t  shim_len;            /* s: 0..48, a multiple of 4 */
    uint8_t  flags;               /* nffacl_adj_flags */
    uint8_t  shim[48];            /* template of output bytes [14, 14 + s) */
} nffacl_adj;
enum nffacl_rewrite_status { NFFACL_RW_APPLIED = 1u, NFFACL_RW_TTL_DONE = 2u, NFFACL_RW_TTL_EXPIRED = 4u };
/* d_hop[0..n): one next hop per SOURCE frame — exactly the d_next that
 * nffacl_lpm_lookup_*_device writes; only its low 24 bits are significant, as
 * in Lookup (choose miss_value >= n_adj for "no rewrite").  d_adj[0..n_adj):
 * device memory the caller fills, n_adj <= 2^24; may be NULL when n_adj is 0.
 * d_status: NULL, or one byte (nffacl_rewrite_status bits) written per j < m.
 * For output frame j: i = d_index[j]; i >= n gives the empty frame, status 0.
 * Else L = the source length, h = d_hop[i], A = d_adj[h], s = A.shim_len.  The
 * record APPLIES iff h < n_adj, L >= 14, s % 4 == 0, s <= 48, A.flags has no
 * unknown bit, every flag's prerequisite above holds, and L + s <= 65535 —
 * decided from d_desc, d_hop and the record alone, never from frame bytes.
 * If it does not apply the frame is copied whole, bit-identical to
 * nffacl_route_gather_frames_device, status 0.  If it applies: L' = L + s,
 * d_out_desc[j] = off_j << 16 | L', the room is L' rounded up to `align`, pads
 * zeroed, status has APPLIED, and the output bytes are
 *   [0, 12)      dmac, smac under MACS, else the source's
 *   [12, 14)     ether_type big-endian if s > 0 and ether_type != 0, else the source's
 *   [14, 14+s)   the shim template, then in this order
 *                  INNER_ETYPE  shim [s-2, s) <- source bytes 12-13
 *                  GTP_LEN      shim [30, 32) <- L - 14, big-endian (gtp.go:118, 125)
 *                  UDP_LEN      shim [24, 26) <- L' - 34; the UDP checksum stays
 *                               what the template holds (the example sends 0)
 *                  IP4_LEN      shim [2, 4) <- L' - 14; last, shim [10, 12) <-
 *                               ~fold of the ten big-endian words of shim [0, 20)
 *                               as they leave, the field taken as 0 (fold =
 *                               reduceChecksum, checksum.go:179-184)
 *   [14+s, L')   source bytes [14, L), under TTL with this edit:
 *                  IPv4 (source EtherType 0x0800, version nibble at byte 14 = 4,
 *                  IHL >= 5, L >= 34): TTL >= 2 -> TTL - 1 and HdrChecksum' =
 *                  ~fold(~HC + ~m + m') (RFC 1624 eq. 3; m = the big-endian word
 *                  (TTL, protocol)), status gets TTL_DONE; TTL <= 1 -> nothing
 *                  changes, status gets TTL_EXPIRED (the frame is still
 *                  encapsulated: the caller drops or diverts it by the status)
 *                  IPv6 (0x86DD, nibble 6, L >= 54): the same rule on the hop
 *                  limit (byte 21), no checksum
 *                  anything else: neither bit
 * A record that applies with s = 0 and flags = 0 yields the plain gather's bytes.
 * Divergences from the reference: examples/gtpu.go:91 stores DgramLen unswapped,
 * here every length is big-endian; decrementTTL.go leaves the header checksum
 * to the NIC, here it is patched.
 * Everything else — packing, align 16..4096, out_cap, *d_out_bytes, repeated
 * indices, m <= max_n, m = 0, three launches on `stream`, no allocation, no
 * global atomics, no memset (capturable), the router's event and one-stream
 * rule, the scratch (nffacl_route_frames_plan), a 16-byte source chunk read
 * only if it starts inside its frame, nothing written at or past out_cap — is
 * as nffacl_route_gather_frames_device.  d_frames, d_out and d_adj 16-byte,
 * d_hop 4-byte aligned.  NFFACL_ERR_INVALID_ARG, with no launch, for a bad
 * align or out_cap, NULL or misaligned buffers, d_hop NULL with n > 0, d_adj
 * NULL with n_adj > 0, n_adj > 2^24, m > max_n. */
NFFACL_API int nffacl_route_gather_encap_frames_device(nffacl_router *r, const uint8_t *d_frames,
                                                       const uint64_t *d_desc, uint64_t n, const uint32_t *d_hop,
                                                       const nffacl_adj *d_adj, uint32_t n_adj,
                                                       const uint32_t *d_index, uint64_t m, uint32_t align,
                                                       uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_desc,
                                                       uint64_t *d_out_bytes, uint8_t *d_status, void *stream);
/* Their plan (pure, no device): tiles = ceil(m / frames-per-tile);
 * scratch_bytes = what a router of max_n = m holds for this path (one 64-bit
 * sum per tile).  NFFACL_ERR_INVALID_ARG for m > 2^31 or NULL outputs. */
NFFACL_API int nffacl_route_frames_plan(uint64_t m, uint64_t *tiles, uint64_t *scratch_bytes);
/* Waits for the router's last launch (its own event, no device-wide
 * synchronise), then frees. */
NFFACL_API void nffacl_router_destroy(nffacl_router *r);

/* ---- longest-prefix-match next hops -----------------------------------------
 * CreateLPM / (*LPM).Add / Delete / Lookup / Free (packet/packet.go:857-912,
 * DPDK's rte_lpm): the route table between a key's destination address and
 * nffacl_route_device, for a batch resident in HBM.  Additive to ABI 7.
 *
 * The prefix of a rule is the top `depth` bits of the u32 value, exactly as
 * Lookup computes ip >> 8.  The reference is handed ipv4.DstAddr as it lies in
 * the header (a types.IPv4Address, first octet in the low byte), so it counts
 * bits from the LAST octet; that is the default here too.
 * NFFACL_LPM_SWAP_BYTES byte-swaps each looked-up address before the walk, so
 * that a types.IPv4Address out of a key is matched from its first octet
 * against rules given as host-order numbers.
 *
 * Divergence: the reference's Add / Delete are visible to the next Lookup.
 * Here they change the host rule list only; nffacl_lpm_commit compiles the
 * list from scratch into a device table and makes it the active one, and a
 * lookup uses the table of the last commit (examples/netlink.go updates its
 * table in batches anyway).  A retired table is freed stream-ordered behind
 * the launches that still read it, with no device synchronise.
 *
 * The device table is not DIR-24-8 but 16-8-8: 65 536 u16 top-level entries
 * that a workgroup stages into LDS (a leaf names one of up to 4 095 next hops
 * held beside them), and 256-entry groups in HBM for prefixes longer than 16
 * and 24.  A table whose level-1 groups (a /16 block holding a longer prefix,
 * or a /16 leaf past the 4 095 coded hops) outnumber 65 535 - H, H the coded
 * hops, does not commit: NFFACL_ERR_NOMEM.
 *
 * Thread-safe: the rule list and the active table are guarded by one lock;
 * lookups may run concurrently with add / delete / commit. */
typedef struct nffacl_lpm nffacl_lpm;
enum nffacl_lpm_flags {
    NFFACL_LPM_SWAP_BYTES = 1u,   /* bswap32 every address before the walk */
    NFFACL_LPM_FORCE_LDS = 2u,    /* the form that stages the top level in LDS, whatever n */
    NFFACL_LPM_FORCE_GLOBAL = 4u  /* the form that reads it from global memory (not both) */
};
/* CreateLPM(name, socket, maxRules, numberTbl8); name and socket have no
 * meaning here.  max_rules >= 1. */
NFFACL_API int nffacl_lpm_create(uint32_t max_rules, uint32_t number_tbl8, nffacl_lpm **out);
/* depth 1..32, else NFFACL_ERR_INVALID_ARG.  ip is masked to depth, next_hop
 * keeps its low 24 bits (Lookup's & 0x00FFFFFF).  An existing (masked ip,
 * depth) has its next hop replaced.  NFFACL_ERR_NOMEM when the rule count
 * would pass max_rules, or the distinct /24 blocks holding a prefix longer
 * than 24 would pass number_tbl8 (rte_lpm's tbl8 budget, checked here). */
NFFACL_API int nffacl_lpm_add(nffacl_lpm *lpm, uint32_t ip, uint32_t depth, uint32_t next_hop);
/* NFFACL_ERR_INVALID_ARG when (masked ip, depth) is not in the list. */
NFFACL_API int nffacl_lpm_delete(nffacl_lpm *lpm, uint32_t ip, uint32_t depth);
NFFACL_API int nffacl_lpm_count(const nffacl_lpm *lpm, uint64_t *rules);
NFFACL_API void nffacl_lpm_free(nffacl_lpm *lpm);
/* Compile the rule list and make the result the active table on hip_device
 * (every commit of one nffacl_lpm names the same device). */
NFFACL_API int nffacl_lpm_commit(nffacl_lpm *lpm, int hip_device);

/* The compiled table without a device (tooling and tests).  Blob, in dwords:
 * [0] magic  [1] H  [2] level-1 groups  [3] level-2 groups  [4] off_l0
 * [5] off_hops  [6] off_l1  [7] off_l2.  L0: 65 536 u16 by address bits
 * 31..16 (0 miss, 1..H leaf with answer word hops[e], above H level-1 group
 * e - H - 1).  Answer and group words: bit 31 hit, bit 30 (level 1 only)
 * level-2 group number in the low 24 bits, else the next hop there.  Groups
 * are 256 words, level 1 by bits 15..8, level 2 by bits 7..0.  *need_dwords
 * is always set; blob may be NULL; cap_dwords too small with a blob is
 * NFFACL_ERR_INVALID_ARG. */
NFFACL_API int nffacl_lpm_compile(const nffacl_lpm *lpm, uint32_t *blob, uint64_t cap_dwords,
                                  uint64_t *need_dwords);

/* d_next[i] (may be NULL) <- the next hop of d_addr[i], or miss_value on a
 * miss; bit i of d_hit_bits (may be NULL; ceil(n / 64) words, the last word's
 * spare bits 0) <- Lookup's bool.  d_next can go straight into
 * nffacl_route_device.  Arrays 16-byte aligned, n < 2^32; nothing past n is
 * read or written.  Asynchronous on `stream`; no atomics, no allocation, no
 * memset: a launch may be captured and replayed while the table it was issued
 * against is still the active one (a commit retires it).
 * NFFACL_ERR_INVALID_ARG, with no launch: no commit yet, both outputs NULL,
 * unknown flags or both FORCE flags, NULL or misaligned arrays, n >= 2^32. */
NFFACL_API int nffacl_lpm_lookup_device(nffacl_lpm *lpm, const uint32_t *d_addr, uint64_t n, uint32_t flags,
                                        uint32_t miss_value, uint32_t *d_next, uint64_t *d_hit_bits,
                                        void *stream);
/* The same for the b field (destination) of family-4 keys; a key of any other
 * family misses, and nothing outside d_keys[0, n) is read. */
NFFACL_API int nffacl_lpm_lookup_keys_device(nffacl_lpm *lpm, const nffacl_key *d_keys, uint64_t n,
                                             uint32_t flags, uint32_t miss_value, uint32_t *d_next,
                                             uint64_t *d_hit_bits, void *stream);

/* ---- misc ------------------------------------------------------------- */
NFFACL_API const char *nffacl_strerror(int status);
NFFACL_API int nffacl_abi_version(void);
/* Last HIP / engine error message recorded on this thread ("" if none). */
NFFACL_API const char *nffacl_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* NFFACL_H */
