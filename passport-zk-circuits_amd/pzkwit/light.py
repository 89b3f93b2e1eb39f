"""RegisterIdentityLight(DG_HASH_TYPE, DOCUMENT_TYPE) inputs (identityManagement/registerIdentityLight.circom:15-92):
the input row, the circuit's three outputs restated with hashlib / Poseidon / BabyJubJub, and rows for the rate
script (tools/light_rate.py).

Row layout = main's input declaration order (1025 elements of 32 B, little-endian, normal form): dg1[1024] (the
DG1 padded for DG_HASH_TYPE's hash: two 512-bit blocks up to SHA-256, one 1024-bit block above), skIdentity.
"""
import numpy as np

from . import inputs as I
from .field import P, SplitMix64, poseidon
from .query import bjj_mul

N_INPUTS = 1025
GROUPS = [("dg1", 0, 1024), ("skIdentity", 1024, 1)]  # (name, offset, length): pzk_instance_input's table
DG_HASHES = (160, 224, 256, 384, 512)


def block_bits(dg_hash):
    """HASH_BLOCK_SIZE (registerIdentityLight.circom:30-35)."""
    return 1024 if dg_hash > 256 else 512


def chunk_bits(doc):
    """DG1_CHUNK_SIZE (registerIdentityLight.circom:40-43)."""
    return 190 if doc == 1 else 186


def dg1_bits(dg1_bytes, dg_hash):
    """The 1024 dg1 input bits of a DG1: SHA padding for the hash's block size (process_passport.js)."""
    bits = I.padded_bits(dg1_bytes, block_bits(dg_hash))
    if len(bits) != 1024:
        raise ValueError("DG1 of %d bytes pads to %d bits, not 1024" % (len(dg1_bytes), len(bits)))
    return bits


def pack(dg1_bytes, sk, dg_hash, out=None):
    """(DG1 bytes, skIdentity, DG_HASH_TYPE) -> (1025, 32) uint8 row."""
    row = out if out is not None else np.zeros((N_INPUTS, 32), dtype=np.uint8)
    row[:] = 0
    row[:1024, 0] = dg1_bits(dg1_bytes, dg_hash)
    row[1024] = np.frombuffer((int(sk) % P).to_bytes(32, "little"), dtype=np.uint8)
    return row


def public_outputs(dg1_bytes, sk, dg_hash, doc):
    """(dg1Commitment, dg1Hash, pkIdentityHash): Poseidon5(4 x Bits2Num(CH) of the dg1 bits, Poseidon1(sk)); the
    digest read as a big-endian integer mod 2^248; Poseidon2(sk * Base8)."""
    bits = [int(b) for b in dg1_bits(dg1_bytes, dg_hash)]
    ch = chunk_bits(doc)
    chunks = [sum(bits[i * ch + j] << j for j in range(ch)) for i in range(4)]
    commit = poseidon(chunks + [poseidon([sk % P])])
    digest = int.from_bytes(I.HASHES[dg_hash](dg1_bytes).digest(), "big") % (1 << 248)
    ax, ay = bjj_mul(sk % P)
    return commit, digest, poseidon([ax, ay])


def batch_rows(batch, seed=0x11, dg_hash=256, doc=3, distinct=64):
    """(batch, 1025, 32) rows: `distinct` synthetic DG1s (93 bytes for TD3, 95 for TD1) with random keys, repeated."""
    rng = SplitMix64(seed)
    n = 95 if doc == 1 else 93
    head = bytes.fromhex("615d5f1f5a" if doc == 1 else "615b5f1f58")
    mrz = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789<"
    uniq = []
    for _ in range(min(batch, distinct)):
        dg1 = head + bytes(mrz[rng.below(len(mrz))] for _ in range(n - len(head)))
        uniq.append(pack(dg1, rng.fr(), dg_hash))
    out = np.empty((batch, N_INPUTS, 32), dtype=np.uint8)
    for i in range(batch):
        out[i] = uniq[i % len(uniq)]
    return out
