/* pzkwit.h — C-ABI of the MI355X batched witness generator (libpzkwit.so).
 *
 * Drop-in boundary for the witness-calculation surface of the reference:
 *   - circom's generated witness calculator, used by circom_tester
 *     (test/automatisationTest.js:37-51: wasm_tester -> circuit.calculateWitness(input, true))
 *     and by generate_witness.js (circuits/scripts/gen-witness.sh:25 -> calculateWTNSBin);
 *   - the per-input serial loop of test/automatisationTest.js:24, replaced by one batched call.
 * The JS binding (passport-zk-circuits_amd/js, Node N-API) and the Python binding
 * (passport-zk-circuits_amd/pzkwit) sit on top of these entry points; INTEGRATION.md shows
 * the bindings a maintainer adds.
 *
 * Conventions: plain pointers and sizes; every function returns 0 on success or a negative
 * PZK_E_* code, with a message in pzk_last_error() (thread-local). Caller owns all input and
 * output buffers; the instance owns its device scratch. Calls on one instance are serialised by an
 * internal mutex (concurrent callers wait); every call runs on the instance's device, whatever the
 * calling thread's current device (which is restored on return).
 * Field elements are 32 bytes, little-endian, NORMAL form (< p), as in a .wtns file.
 */
#ifndef PZKWIT_H
#define PZKWIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* circuit families (the `component main` the instance evaluates) */
enum {
  PZK_CIRCUIT_REGISTER = 0, /* RegisterIdentityBuilder(...)  registerIdentityBuilder.circom:41 */
  PZK_CIRCUIT_POSEIDON = 1, /* PoseidonHash(n)               poseidon.circom:214 (config 1) */
  PZK_CIRCUIT_SHA256 = 2,   /* Sha256HashChunks(blocks)      sha256HashChunks.circom:8 (config 2) */
  PZK_CIRCUIT_SHA1 = 3,     /* Sha1HashChunks(blocks)        hasher/sha1/sha1.circom:7 */
  PZK_CIRCUIT_SHA384 = 4,   /* Sha384HashChunks(blocks)      hasher/sha2/sha384/sha384HashChunks.circom:8 */
  PZK_CIRCUIT_SHA512 = 5,   /* Sha512HashChunks(blocks)      hasher/sha2/sha512/sha512HashChunks.circom */
  PZK_CIRCUIT_QUERY = 6,    /* QueryIdentity(idTreeDepth = size_arg, 80)  identityManagement/queryIdentity.circom:37;
                               BabyPbk (undefined in the snapshot) is the reference's BabyjubjubBase8Multiplication,
                               DESIGN.md §11 */
  PZK_CIRCUIT_LIGHT = 7     /* RegisterIdentityLight(dg_hash_type, document_type)
                               identityManagement/registerIdentityLight.circom:15; dg_hash_type 160, 224, 256, 384 or
                               512, document_type 1 or 3, every other pzk_params field ignored; inputs dg1[1024],
                               skIdentity; outputs dg1Commitment, dg1Hash, pkIdentityHash; no public inputs (the
                               reference declares no main). BabyPbk as for QUERY, DESIGN.md §13 */
};

/* Template parameters of RegisterIdentityBuilder (registerIdentityBuilder.circom:41-52),
 * verbatim, plus the circuit family and its size argument for the standalone circuits. */
typedef struct pzk_params {
  int32_t circuit;            /* PZK_CIRCUIT_* */
  int32_t size_arg;           /* n for POSEIDON, blocks for SHA256 / SHA1 / SHA384 / SHA512, idTreeDepth (80) for
                                 QUERY; ignored for REGISTER */
  int32_t signature_type;     /* SIGNATURE_TYPE (signatureVerification.circom:9-127): 1 = RSA-2048 PKCS#1 v1.5
                                 SHA-256 e = 65537, 2 = RSA-4096, 3 = RSA-2048 SHA-1, 4 = RSA-3072 SHA-1
                                 e = 37187; 10-12 = RSA-2048 PSS SHA-256 (10: e = 3; 12: salt 64), 13 = RSA-2048
                                 PSS SHA-384 (salt 48), 14 = RSA-3072 PSS SHA-256; 20 = ECDSA secp256r1,
                                 21 = ECDSA brainpoolP256r1 (SHA-256), 24 = ECDSA secp224r1 (7 x 32-bit chunks;
                                 SHA-224 signed attributes, SHA-256 encapsulated content), 25 = ECDSA
                                 brainpoolP384r1 (6 x 64-bit chunks, SHA-384). 22 / 23 do not compile in the
                                 reference (ecdsa.circom:31-37 reads past hashed[]). Others: PZK_E_PARAMS */
  int32_t dg_hash_type;       /* DG_HASH_TYPE (160, 224, 256, 384; LIGHT: also 512) */
  int32_t document_type;      /* DOCUMENT_TYPE (1 = TD1, 3 = TD3) */
  int32_t ec_block_number;    /* EC_BLOCK_NUMBER */
  int32_t ec_shift;           /* EC_SHIFT (bits) */
  int32_t dg1_shift;          /* DG1_SHIFT (bits) */
  int32_t aa_signature_algo;  /* AA_SIGNATURE_ALGO (0 = none, 1..19 = RSA-1024 key, 20..25 = EC key) */
  int32_t dg15_shift;         /* DG15_SHIFT (bits) */
  int32_t dg15_block_number;  /* DG15_BLOCK_NUMBER */
  int32_t aa_shift;           /* AA_SHIFT (bits) */
} pzk_params;

typedef struct pzk_info {
  uint64_t witness_size;   /* number of field elements per witness (wtns section 2 / 32) */
  uint64_t n_inputs;       /* number of input signals (flat input buffer length / 32) */
  uint32_t n_outputs;      /* main outputs (witness[1 .. n_outputs]) */
  uint32_t n_public_inputs;/* public inputs, right after the outputs */
  uint32_t n_input_groups; /* named input signals (see pzk_instance_input) */
  uint32_t pipeline_depth; /* calls in flight with a NULL stream: call k + pipeline_depth starts after call k
                              has completed (pzk_witness_batch) */
} pzk_info;

typedef struct pzk_exec {
  int32_t device;   /* HIP device ordinal: must be the instance's device, or < 0 for "the instance's" */
  int32_t flags;    /* PZK_EXEC_* */
  void* stream;     /* hipStream_t the call is ordered after and joined into at exit (serialises calls);
                       NULL = the instance's own streams, pipelined across calls: complete after
                       pzk_instance_sync() (or PZK_EXEC_SYNC / a device-wide synchronise) */
} pzk_exec;

enum {
  PZK_EXEC_SYNC = 1,   /* synchronise the stream before returning */
  PZK_EXEC_TIMING = 2  /* bracket every kernel phase with HIP events on the launch stream */
};

/* lane status codes: 0 = OK, else the first failing `===` site (reference file:line) */
enum {
  PZK_ST_OK = 0,
  PZK_ST_NUM2BITS = 1,    /* bitify.circom:26 */
  PZK_ST_ALIAS = 2,       /* aliascheck.circom:14 */
  PZK_ST_ISZERO = 3,      /* comparators.circom:20 */
  PZK_ST_LASTBIT = 4,     /* int/arithmetic.circom:169-170 */
  PZK_ST_LASTNBITS = 5,   /* int/arithmetic.circom:203 */
  PZK_ST_BITS2 = 6,       /* sha2Common.circom:65-68 */
  PZK_ST_FLOW = 7,        /* passportVerificationBuilder.circom:155 */
  PZK_ST_RSA_HASH = 8,    /* rsa.circom:48 */
  PZK_ST_RSA_PREFIX = 9,  /* rsa.circom:53-54 */
  PZK_ST_RSA_PAD = 10,    /* rsa.circom:57-71 */
  PZK_ST_BIGMOD_GT = 11,  /* bigInt.circom:245 */
  PZK_ST_BIGISZERO = 12,  /* bigIntComparators.circom:128 */
  PZK_ST_SMT_LAST = 13,   /* SMTVerifier.circom:54 */
  PZK_ST_BJJ_ADD = 14,    /* babyjubjub/curve.circom:98,102 */
  PZK_ST_ECDSA_INV = 15,  /* bigInt.circom:364-368 (in * inv mod n === 1) */
  PZK_ST_ECDSA_R = 16,    /* ecdsa.circom:81-83 (x1 mod n === r) */
  PZK_ST_PSS_TRAILER = 17,/* rsaPss.circom:73 (assert eM[0] == 188) */
  PZK_ST_PSS_HASH = 18,   /* rsaPss.circom:182,201 (hDash256.out === hash) */
  PZK_ST_QUERY = 19,      /* comparators.circom:42 ((1 - isEqual.out) * enabled === 0: a selected query bound fails) */
  PZK_ST_DATE = 20,       /* dateDecoder.circom:22 (encoded === dateEncoded: not a "YYMMDD" digit string) */
  PZK_ST_CIT_BLACKLIST = 21, /* citizenshipCheck.circom:271 (the citizenship is in the mask) */
  PZK_ST_CIT_LIST = 22,   /* citizenshipCheck.circom:274 (the citizenship is not in COUNTRY_ARR) */
  PZK_ST_ISV_ROOT = 23,   /* identityStateVerifier.circom:46 (smtVerifier.isVerified === 1) */
  PZK_ST_INPUT_RANGE = 64 /* an input outside the domain the GPU path evaluates: a non-bit SHA input, a
                             limb >= 2^64, a field scalar >= p (skIdentity, the SMT root and siblings,
                             eventID, eventData, pkPassportHash: raw bytes are not reduced). Other
                             lanes of the batch are not affected; a lane that also fails a circuit
                             check reports that smaller code. See DESIGN.md §5 */
};

enum {
  PZK_E_ARG = -1,       /* invalid argument */
  PZK_E_PARAMS = -2,    /* unsupported template parameters */
  PZK_E_HIP = -3,       /* HIP runtime error */
  PZK_E_NOMEM = -4,     /* device allocation failed */
  PZK_E_DATA = -5,      /* Poseidon parameter file missing/corrupt */
  PZK_E_NODEVICE = -6   /* no HIP device: the library never falls back to a CPU path */
};

typedef struct pzk_instance pzk_instance;

/* Replaces: circom compile + WitnessCalculator builder(wasm) — witness_calculator.js builder(). */
int pzk_instance_create(const pzk_params* params, pzk_instance** out);
void pzk_instance_destroy(pzk_instance* inst);

/* Same, with a signal -> witness map in circom's .sym format (circom --sym: one line per signal,
 * "signal_idx,witness_idx,component_idx,name", witness_idx = -1 for a signal the compiler eliminated;
 * signal indices in the --O0 numbering of DESIGN.md §2). The instance's witness is then the mapped
 * one: witness_size = number of kept signals + 1, element k = the O0 signal whose witness_idx is k,
 * and the .wtns header reports that size. sym = NULL is pzk_instance_create (the identity map).
 * Replaces: the witness layout circom --O1/--O2 bakes into the WASM (circuits/scripts/compile-circuit.sh:34). */
int pzk_instance_create_mapped(const pzk_params* params, const char* sym, size_t sym_len, pzk_instance** out);
/* Host-only: validate a .sym against an instance's O0 numbering; *witness_size = mapped size. */
int pzk_sym_check(const pzk_params* params, const char* sym, size_t sym_len, uint64_t* witness_size);

/* Host-only layout queries (no device needed): witness/input sizes of an instance and its
 * emit-region table (offset, length, kind). Used by the CPU test suite. */
int pzk_layout_query(const pzk_params* params, pzk_info* info, uint32_t* n_regions);
int pzk_layout_region(const pzk_params* params, uint32_t i, uint64_t* off, uint32_t* len, uint32_t* kind);

/* Replaces: wc.witnessSize / wc.n32 / wc.prime fields and getInputSignalSize(fnv(name)). */
int pzk_instance_info(const pzk_instance* inst, pzk_info* info);
/* i-th named input signal, in flat-input order: name, element offset and length. */
int pzk_instance_input(const pzk_instance* inst, uint32_t i, const char** name, uint64_t* offset,
                       uint64_t* length);

/* ---- Packed input rows ----
 * A full input row spends 32 bytes on every input, though most inputs are one bit or one 64-bit limb. The
 * packed row holds the same groups (pzk_instance_input), in the same order, each at a multiple of 16 bytes:
 *   PZK_INPUT_BIT   n inputs in ceil(n / 8) bytes, input j = bit 7 - (j & 7) of byte j >> 3 (MSB first: a hashed
 *                   message's padded bytes verbatim); pad bits are written 0 and ignored
 *   PZK_INPUT_LIMB  8 bytes little-endian per input
 *   PZK_INPUT_FIELD the 32 bytes verbatim (a scalar >= p stays representable and reports PZK_ST_INPUT_RANGE)
 * every group and the row padded to a multiple of 16 bytes. The packed entry points expand the rows on the GPU
 * (k_unpack_inputs) into the 32-byte rows every other kernel reads; the unpacked entry points are unchanged and
 * remain the path for rows outside the packed domain (a non-bit in a BIT group, a limb >= 2^64). */
enum { PZK_INPUT_BIT = 0, PZK_INPUT_LIMB = 1, PZK_INPUT_FIELD = 2 };

/* Host-only: bytes per packed row of an instance, and the i-th group's kind, byte offset in the packed row and
 * byte length (without the padding to 16). Groups are indexed as in pzk_instance_input. */
int pzk_packed_layout(const pzk_params* params, uint64_t* row_bytes);
int pzk_packed_group(const pzk_params* params, uint32_t i, uint32_t* kind, uint64_t* byte_offset,
                     uint64_t* byte_length);
/* The same for a live instance. */
int pzk_instance_input_packed(const pzk_instance* inst, uint32_t i, uint32_t* kind, uint64_t* byte_offset,
                              uint64_t* byte_length);

/* Host: pack n full rows (n x n_inputs x 32 B) into packed rows (n x row_bytes) on `threads` host threads
 * (<= 0: all this process may use). status = n x int32 (may be NULL): 0, or 1 for a row that has no packed form
 * (a BIT input other than 0 / 1, a LIMB input >= 2^64); such a row's packed row is zero-filled, and the row
 * stays on the unpacked path, where the GPU flags it. */
int pzk_pack_inputs(const pzk_params* params, const uint8_t* rows, size_t n, uint8_t* packed, int32_t* status,
                    int threads);
/* Host: the inverse, packed rows -> full rows (n x n_inputs x 32 B). The CPU reference of the GPU kernel. */
int pzk_unpack_inputs_host(const pzk_params* params, const uint8_t* packed, size_t n, uint8_t* rows);

/* Device packed rows (batch x row_bytes, 16-byte aligned) -> caller-owned device full rows (batch x n_inputs x
 * 32 B, 16-byte aligned), on exec->stream (NULL: the instance's main stream; complete after pzk_instance_sync or
 * PZK_EXEC_SYNC). A caller that reuses inputs expands them once and calls pzk_witness_batch on the rows. */
int pzk_unpack_inputs(pzk_instance* inst, const uint8_t* d_packed, size_t batch, uint8_t* d_rows,
                      const pzk_exec* exec);

/* The 76-byte .wtns header (wtns v2, 2 sections, n8 = 32, prime, witnessSize) that
 * calculateWTNSBin prepends. */
int pzk_wtns_header(const pzk_instance* inst, uint8_t header[76]);

/* Batched witness calculation on device buffers (inputs resident in HBM).
 *   d_inputs : batch x n_inputs x 32 B (normal form), device pointer
 *   d_wtns   : batch x witness_size x 32 B elements, row stride wtns_stride bytes (>= 32*witness_size,
 *              multiple of 16), device pointer
 *   d_status : batch x int32 lane status (PZK_ST_*), device pointer (may be NULL)
 * The buffers must stay untouched until the call has completed (see pzk_exec.stream). With a NULL
 * stream consecutive calls overlap: the instance keeps pzk_info.pipeline_depth (3) scratch sets, call
 * k uses set k mod 3, so calls k, k + 1 and k + 2 may run at the same time (call k + 1's cores beside
 * call k's emitters) and call k + 3 starts after call k has completed. A caller that reuses call k's
 * d_inputs / d_wtns / d_status for a later call must therefore either give the later call an index
 * >= k + 3 or synchronise first (pzk_instance_sync, PZK_EXEC_SYNC, or a stream).
 * Replaces: for (input of inputs) await wc.calculateWitness(input) (automatisationTest.js:24-50). */
int pzk_witness_batch(pzk_instance* inst, const uint8_t* d_inputs, size_t batch, uint8_t* d_wtns,
                      size_t wtns_stride, int32_t* d_status, const pzk_exec* exec);

/* Wait until every call issued on the instance so far has completed (all instance streams). */
int pzk_instance_sync(pzk_instance* inst);

/* Host-buffer convenience (copies in/out; used by the single-input calculateWitness path). */
int pzk_witness_batch_host(pzk_instance* inst, const uint8_t* h_inputs, size_t batch, uint8_t* h_wtns,
                           int32_t* h_status, const pzk_exec* exec);

/* pzk_witness_batch / pzk_witness_batch_host on packed rows (d_packed / h_packed: batch x row_bytes of
 * pzk_packed_layout; device pointer 16-byte aligned). Same contract: stream semantics, pipelining over the scratch
 * sets, batch limit, statuses. The rows are expanded into the call's scratch set first (allocated at an instance's
 * first packed call), on the call's chain stream, and every kernel then runs as in the unpacked call. */
int pzk_witness_batch_packed(pzk_instance* inst, const uint8_t* d_packed, size_t batch, uint8_t* d_wtns,
                             size_t wtns_stride, int32_t* d_status, const pzk_exec* exec);
int pzk_witness_batch_host_packed(pzk_instance* inst, const uint8_t* h_packed, size_t batch, uint8_t* h_wtns,
                                  int32_t* h_status, const pzk_exec* exec);

/* Streamed delivery to host memory (replaces gen-witness.sh's one generate_witness.js + .wtns write per
 * input, circuits/scripts/gen-witness.sh:25, for a whole batch): h_inputs = batch x n_inputs x 32 B (host);
 * the batch runs in chunks of `chunk` witnesses (0: ~4 GiB of rows per chunk), and as each chunk's rows
 * arrive in pinned host memory the calling thread passes them to
 *   sink(user, first, n, rows, row_stride, status): rows[i * row_stride ..] is witness first + i (32 B
 *   elements, witness_size of them; the .wtns section 2 payload), status[i] its lane status.
 * The rows are valid only during the call (the buffer is reused two chunks later); a non-zero return stops
 * the stream (PZK_E_ARG). Chunk c + 1 computes and chunk c copies down while the sink runs on chunk c - 1,
 * so a sink that keeps up leaves the host link (PCIe) as the bound. */
typedef int (*pzk_sink_fn)(void* user, size_t first, size_t n, const uint8_t* rows, size_t row_stride,
                           const int32_t* status);
int pzk_witness_stream(pzk_instance* inst, const uint8_t* h_inputs, size_t batch, size_t chunk, pzk_sink_fn sink,
                       void* user, const pzk_exec* exec);

/* ---- Checking witness rows against a circom .r1cs file ----
 * Replaces: circuit.checkConstraints(w) (test/automatisationTest.js:51), for a whole batch of rows resident in HBM.
 * The file is circom's / snarkjs' binary format, version 1, over BN254's scalar field: a header section (type 1), a
 * constraint section (type 2), optionally a wire-to-label section (type 3); sections in any order, other types
 * skipped. Within a linear combination wires may come in any order and more than once (their coefficients add), and
 * a coefficient may be 0. Rejected with PZK_E_ARG: wrong magic, version != 1, fieldSize != 32, another prime, a
 * missing or duplicate type-1 or type-2 section, any size that runs past the buffer or its section, trailing bytes
 * in the constraint section, a wire id >= nWires, a coefficient >= p, nWires = 0, a type-3 section that is not
 * 8 * nWires bytes, mConstraints >= 2^31 (a constraint index fits the int32 result). */
typedef struct pzk_r1cs pzk_r1cs;
typedef struct pzk_r1cs_info {
  uint32_t n_wires, n_pub_out, n_pub_in, n_prv_in;
  uint64_t n_labels;
  uint32_t n_constraints, n_long; /* n_long: constraints on the wave-per-constraint path (an LC of more than 32 terms) */
  uint64_t n_terms;               /* after merging duplicate wires and dropping zero coefficients */
  uint32_t n_coeffs, max_terms;   /* entries of the coefficient table: the distinct coefficients in use and the two
                                     fixed entries 1 and p - 1; terms of the longest LC */
} pzk_r1cs_info;

/* Host only (no device needed); the program is uploaded at the object's first check. */
int pzk_r1cs_load(const uint8_t* bytes, size_t len, pzk_r1cs** out);
void pzk_r1cs_destroy(pzk_r1cs* r);
int pzk_r1cs_get_info(const pzk_r1cs* r, pzk_r1cs_info* info);

/* Check batch rows against the system on the GPU.
 *   d_wtns         : batch rows of stride bytes (>= 32 * n_wires, a multiple of 16; device pointer 16-byte aligned),
 *                    32 B little-endian per wire, as pzk_witness_batch writes them. An element >= p counts as its
 *                    residue. Bytes past 32 * n_wires of a row are not read.
 *   d_first_failed : batch x int32: -1 = every constraint holds, k >= 0 = the lowest index (file order) of a violated
 *                    constraint
 *   d_n_failed     : batch x uint32 violated constraints per row; may be NULL
 * exec->stream: the check is ordered after it and runs on it. NULL: the object's own stream (the caller has
 * synchronised whatever wrote the rows; complete after PZK_EXEC_SYNC or a device-wide synchronise). The object is
 * bound to the device of its first check (exec->device, or < 0 / exec NULL: the current device); calls on one object
 * are serialised by an internal mutex. batch = 0 returns 0. Without a device: PZK_E_NODEVICE. */
int pzk_r1cs_check_batch(pzk_r1cs* r, const uint8_t* d_wtns, size_t batch, size_t stride, int32_t* d_first_failed,
                         uint32_t* d_n_failed, const pzk_exec* exec);
/* The same on host buffers (copies in and out; complete on return). */
int pzk_r1cs_check_batch_host(pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, int32_t* first_failed,
                              uint32_t* n_failed, const pzk_exec* exec);
/* The kernels' host twin, as pzk_unpack_inputs_host is k_unpack_inputs': plain C++, one thread, no device, same
 * results. Not a fallback: the two entry points above never call it. */
int pzk_r1cs_eval_host(const pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, int32_t* first_failed,
                       uint32_t* n_failed);

/* ---- Groth16's quotient evaluations for witness rows ----
 * The first stage of `snarkjs groth16 prove` (circuits/scripts/prove.sh:25-27), for a batch of rows resident in HBM.
 * With nC = n_constraints and nPub = n_pub_out + n_pub_in: M = nC + nPub + 1, N = 2^k the smallest power of two >= M
 * (1 <= k <= 24, else PZK_E_ARG). Per row w: a_i = A_i.w and b_i = B_i.w for i < nC; a_(nC + s) = w_s, b_(nC + s) = 0
 * for s = 0 .. nPub; zero from M on; c_i = a_i b_i. Each of a, b, c goes through an inverse transform of N points
 * (factor 1 / N included), coefficient i times g^i, and a forward transform: its evaluations on the coset g <w_N>,
 * where w_(2^28) = 5^((p - 1) / 2^28), w_(2^s) = w_(2^28)^(2^(28 - s)) and g = w_(2N). The result is
 * h_j = a'_j b'_j - c'_j, j < N: natural order, 32 B little-endian, normal form, below p. On a row that violates the
 * system h is still defined by the above, but it is not a quotient: check first. */
typedef struct pzk_quotient_info {
  uint32_t log2_n;        /* k */
  uint32_t tile;          /* witnesses per tile of scratch */
  uint64_t n, n_rows;     /* N, M */
  uint64_t scratch_bytes; /* device memory the object takes at its first quotient call: the b and c vectors of a tile
                             and the transforms' tables */
} pzk_quotient_info;
/* Host only. */
int pzk_r1cs_quotient_info(const pzk_r1cs* r, pzk_quotient_info* info);

/* h for batch rows, on the GPU.
 *   d_wtns : as for pzk_r1cs_check_batch (an element >= p counts as its residue)
 *   d_h    : batch rows of h_stride bytes (>= 32 * N, a multiple of 16; device pointer 16-byte aligned); bytes past
 *            32 * N of a row are not written. The rows are the call's work memory too: they must not overlap d_wtns.
 * Stream, device binding, the mutex, batch = 0 and PZK_E_NODEVICE as for pzk_r1cs_check_batch; on a caller stream
 * nothing synchronises (the object's first quotient call allocates its scratch and builds its tables, and waits for
 * that). Batches above pzk_quotient_info.tile run tile after tile on the same stream. With PZK_EXEC_TIMING the call
 * synchronises after every tile and adds the time of its stages to pzk_r1cs_quotient_timing. */
int pzk_r1cs_quotient_batch(pzk_r1cs* r, const uint8_t* d_wtns, size_t batch, size_t stride, uint8_t* d_h,
                            size_t h_stride, const pzk_exec* exec);
/* The same on host buffers (copies in and out; complete on return). */
int pzk_r1cs_quotient_batch_host(pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, uint8_t* h,
                                 size_t h_stride, const pzk_exec* exec);
/* The kernels' host twin: plain C++, one thread, no device, same bytes. Not a fallback: the two entry points above
 * never call it. */
int pzk_r1cs_quotient_host(const pzk_r1cs* r, const uint8_t* h_wtns, size_t batch, size_t stride, uint8_t* h,
                           size_t h_stride);
/* Milliseconds accumulated by quotient calls made with PZK_EXEC_TIMING: ms[0] the rows a, b, c; ms[1] the three
 * inverse transforms (shift included); ms[2] the forward transforms of a and b; ms[3] the forward transform of c with
 * the pointwise step folded into its last pass. reset != 0 clears them afterwards. */
int pzk_r1cs_quotient_timing(pzk_r1cs* r, double ms[4], int reset);

/* Per-phase kernel time accumulated (ms) by calls made with PZK_EXEC_TIMING, and the number of
 * launches of each phase. On input *count is the capacity of the arrays; on output the number of
 * phases. Synchronises on the recorded events. reset != 0 clears the accumulators afterwards. */
int pzk_timing(pzk_instance* inst, const char** names, double* ms, uint64_t* launches, uint32_t* count, int reset);

/* Static description of a kernel phase: name, kernel symbol, and its ALGORITHMIC HBM bytes per
 * witness (each element written once + the unique bytes it must read). Used for roofline math. */
int pzk_phase_info(const pzk_instance* inst, uint32_t phase, const char** name, const char** kernel,
                   uint64_t* bytes_per_witness);

/* Reason for the last failure on this thread. */
const char* pzk_last_error(void);

/* Library version string. */
const char* pzk_version(void);

#ifdef __cplusplus
}
#endif
#endif
