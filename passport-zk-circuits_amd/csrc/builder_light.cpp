// RegisterIdentityLight(DG_HASH_TYPE, DOCUMENT_TYPE) layout (identityManagement/registerIdentityLight.circom:15-92).
//
// main = RegisterIdentityLight(DG, DOC): the reference declares no main for this template, so no input is public and
// the witness order is the declaration order: outputs (dg1Commitment, dg1Hash, pkIdentityHash), inputs (dg1[1024],
// skIdentity), then the one intermediate array dg1HashBits[DG]. The component tree is walked in creation order like
// builder_register.cpp; the run dg1Hasher .. pkIdentityHasher is the sequence of regions that ends build_register.
// pkIdentityCalc's BabyPbk is the reference's BabyjubjubBase8Multiplication.
#include "builder_impl.hpp"

namespace pzk {

namespace {
uint32_t l_bits(int L) { return 2 * L + 1 + (L == 254 ? 254 + 383 + 271 : 0); }  // Bits2Num / Num2Bits (+ AliasCheck)
}  // namespace

bool build_light(const pzk_params& p, Layout& L, std::string& why) {
  const int DG = p.dg_hash_type;
  if (DG != 160 && DG != 224 && DG != 256 && DG != 384 && DG != 512) {
    why = "RegisterIdentityLight: DG_HASH_TYPE (dg_hash_type) must be 160, 224, 256, 384 or 512";
    return false;
  }
  if (p.document_type != 1 && p.document_type != 3) {
    why = "RegisterIdentityLight: DOCUMENT_TYPE (document_type) must be 1 or 3";
    return false;
  }
  // HASH_BLOCK_SIZE / HASH_BLOCK_NUMBER (:30-35): two 512-bit blocks, or one 1024-bit block above 256-bit hashes
  const int blocks = DG > 256 ? 1 : 2;
  const int chunk = p.document_type == 1 ? 190 : 186;  // DG1_CHUNK_SIZE (:40-43)
  const int IN_DG1 = 0, IN_SK = 1024;

  Builder b(L);
  L.n_inputs = 1025;
  L.n_outputs = 3;
  L.n_public = 0;
  L.inputs = {{"dg1", (uint64_t)IN_DG1, 1024, IK_BIT}, {"skIdentity", (uint64_t)IN_SK, 1}};
  L.is_light = true;
  L.params = p;
  L.bjj_core_fr = BJJ_CORE_FR;

  // ---- value-store slots (Montgomery): the loaded scalar, k_light_prep's outputs, the BabyJubJub key
  const int V_SK = b.value();
  int V_DG1[4];
  for (int i = 0; i < 4; i++) V_DG1[i] = b.value();
  const int V_DG1HASH = b.value();
  const int V_BJJ_X = b.value(), V_BJJ_Y = b.value();
  L.loads.push_back(ValueLoad{V_SK, IN_SK});
  L.reg.v_sk = V_SK; L.reg.v_dg1 = V_DG1[0]; L.reg.v_dg1hash = V_DG1HASH; L.reg.v_bjj = V_BJJ_X;
  L.reg.in_dg1 = IN_DG1;
  L.reg.dg1_chunk = chunk;
  // Poseidon levels: 0 sk hash; 1 dg1 commitment (needs the sk hash and k_light_prep's chunks); 2 pk identity hash
  // (after the BabyJubJub core)

  // =========================== main: [1 | outputs(3) | dg1, skIdentity | dg1HashBits[DG]] ===========================
  b.region(RK_ONE, 1);
  const uint32_t r_out = b.region(RK_VALUE, 3, {-1});  // patched below (non-contiguous slots)
  b.region(RK_INCOPY, L.n_inputs, {0});
  const int J_DG1 = b.hash_job(DG, IN_DG1, blocks);  // dg1ShaHasher's job: its digest is referenced before its regions
  L.reg.j_dg1 = J_DG1;
  b.region(RK_DIGEST, DG, {J_DG1});
  // dg1Hasher is created at its declaration (:39), before dg1Chunking[i]; its 5th input is skIndentityHasher.out
  const size_t dg1_task = L.pos.size();
  const int S_DG1C = b.poseidon(5, {V_DG1[0], V_DG1[1], V_DG1[2], V_DG1[3], -1}, 1);
  for (int i = 0; i < 4; i++) b.region(RK_BITS2NUM, l_bits(chunk), {chunk, 0, IN_DG1 + i * chunk, 1});
  const int S_SKH = b.poseidon(1, {V_SK}, 0);
  L.pos[dg1_task].in_slot[4] = S_SKH;
  // pkIdentityCalc: BabyjubjubBase8Multiplication: out[2] | scalar | getBase8, num2Bits(254), adders/doublers
  b.region(RK_BJJ_OWN, 3 + 2);
  b.region(RK_NUM2BITS, l_bits(254), {254, 0, V_SK});
  b.region(RK_BJJ_STEPS, 46 + 253 * 60);
  const int S_PKID = b.poseidon(2, {V_BJJ_X, V_BJJ_Y}, 2);
  // dg1ShaHasher = ShaHashChunks(blocks, DG) (hash.circom:32-68): wrapper out | in, then the inner hasher's block
  if (L.sha[J_DG1].algo == 1) {
    b.sha1_regions(J_DG1, IN_DG1, blocks, true);
  } else if (L.sha[J_DG1].algo >= 3) {
    b.sha512_regions(J_DG1, IN_DG1, blocks, true);
  } else {
    const int O = DG;  // 224 | 256
    b.region(RK_SHA_OWN, O + 512ull * blocks + O + 512ull * blocks + 256ull * (blocks + 1) + 256, {J_DG1, blocks, IN_DG1, 1, O});
    for (int m = 0; m < blocks; m++) b.region(RK_SHA_BLOCK, SHA_BLOCK_LEN, {J_DG1, m});
  }
  // b2n = Bits2Num(248): in[i] = dg1HashBits[DG - 1 - i] for i < min(248, DG), 0 above (:72-84). The digest bit source
  // reads a negative index as 0, so first bit DG - 1 with stride -1 gives the zero tail of DG 160 / 224 as it is
  b.region(RK_BITS2NUM, l_bits(248), {248, 1, DG - 1, -1, J_DG1});

  L.out_slots = {S_DG1C, V_DG1HASH, S_PKID};
  L.regions[r_out].a[0] = -3;  // explicit slot list
  L.regions[r_out].a[1] = S_DG1C;
  L.regions[r_out].a[2] = V_DG1HASH;
  L.regions[r_out].a[3] = S_PKID;
  b.finalize();
  return true;
}

}  // namespace pzk
