"""The packed input row format (include/pzkwit.h) restated in Python, independent of the library:
the group tables of the instance families, the offsets the format rules give, and a numpy packer. Shared by
tests/test_packed.py (CPU) and tests/test_gpu_packed.py."""
import numpy as np

from pzkwit import inputs as I, native

BIT, LIMB, FIELD = 0, 1, 2


def register_groups(params):
    """[(kind, elements)] of a RegisterIdentityBuilder instance, from its template parameters
    (registerIdentityBuilder.circom:54-70): root, ec, dg1, dg15, sa, signature, pubkey, branches, sk"""
    sig = params["sig"]
    k = 7 if sig == 24 else 6 if sig == 25 else 4 if sig >= 20 else 64 if sig == 2 else 48 if sig in (4, 14) else 32
    limbs = 2 * k if sig >= 20 else k
    hb = 1024 if sig in (13, 25) else 512
    return [(FIELD, 1), (BIT, params["ec_blocks"] * hb), (BIT, 1024), (BIT, params["dg15_blocks"] * hb), (BIT, 1024),
            (LIMB, limbs), (LIMB, limbs), (FIELD, 80), (FIELD, 1)]


def query_groups(td1):
    """QueryIdentity(80): 16 scalars, dg1 (93 or 95 bytes), 80 siblings, timestamp, identityCounter"""
    return [(FIELD, 1)] * 16 + [(BIT, 760 if td1 else 744), (FIELD, 80), (FIELD, 1), (FIELD, 1)]


LIGHT_GROUPS = [(BIT, 1024), (FIELD, 1)]

# SIG 13 with SHA-256 DG hashes and no DG15 (tests/test_capi.py PARAM_SETS): the dg15 group is empty
NO_DG15 = dict(I.instance_params(13), dg_hash=256, aa=0, dg15_blocks=0)

# (id, circuit, size_arg, params, groups)
INSTANCES = [
    ("register_canonical", native.PZK_CIRCUIT_REGISTER, 0, I.CANONICAL, register_groups(I.CANONICAL)),
    ("register_sig2", native.PZK_CIRCUIT_REGISTER, 0, I.instance_params(2), register_groups(I.instance_params(2))),
    ("register_sig20", native.PZK_CIRCUIT_REGISTER, 0, I.instance_params(20), register_groups(I.instance_params(20))),
    ("register_sig24", native.PZK_CIRCUIT_REGISTER, 0, I.instance_params(24), register_groups(I.instance_params(24))),
    ("register_no_dg15", native.PZK_CIRCUIT_REGISTER, 0, NO_DG15, register_groups(NO_DG15)),
    ("query_td3", native.PZK_CIRCUIT_QUERY, 80, {}, query_groups(False)),
    ("query_td1", native.PZK_CIRCUIT_QUERY, 80, {"doc": 1}, query_groups(True)),
    ("light_256_3", native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=256, doc=3), LIGHT_GROUPS),
    ("light_512_1", native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=512, doc=1), LIGHT_GROUPS),
    ("poseidon_2", native.PZK_CIRCUIT_POSEIDON, 2, {}, [(FIELD, 2)]),
    ("sha256_1", native.PZK_CIRCUIT_SHA256, 1, {}, [(BIT, 512)]),
]
BY_ID = {i[0]: i for i in INSTANCES}


def group_bytes(kind, n):
    return (n + 7) // 8 if kind == BIT else 8 * n if kind == LIMB else 32 * n


def layout(groups):
    """the format rules: every group at the next multiple of 16 -> (row_bytes, [(kind, byte offset, byte length)],
    [element offset])"""
    out, el, by, e = [], [], 0, 0
    for kind, n in groups:
        out.append((kind, by, group_bytes(kind, n)))
        el.append(e)
        by += (group_bytes(kind, n) + 15) // 16 * 16
        e += n
    return by, out, el


def pack(groups, rows):
    """numpy packer of in-domain rows (n, n_inputs, 32) -> (n, row_bytes)"""
    row_bytes, lay, el = layout(groups)
    out = np.zeros((rows.shape[0], row_bytes), dtype=np.uint8)
    for (kind, n), (_, off, ln), e in zip(groups, lay, el):
        g = rows[:, e:e + n]
        if kind == BIT:
            out[:, off:off + ln] = np.packbits(g[:, :, 0], axis=1, bitorder="big")
        elif kind == LIMB:
            out[:, off:off + ln] = g[:, :, :8].reshape(rows.shape[0], -1)  # <u8
        else:
            out[:, off:off + ln] = g.reshape(rows.shape[0], -1)
    return out


def edge_rows(groups, batch, seed):
    """rows over the whole packed domain: random bits; limbs with 0 and 2^64 - 1 among random ones; field elements
    with 0, p - 1, p and 2^256 - 1 among random 32-byte strings"""
    from pzkwit.field import P
    rng = np.random.default_rng(seed)
    n_in = sum(n for _, n in groups)
    rows = np.zeros((batch, n_in, 32), dtype=np.uint8)
    e = 0
    fe = [np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8) for v in (0, P - 1, P, (1 << 256) - 1)]
    for kind, n in groups:
        if kind == BIT:
            rows[:, e:e + n, 0] = rng.integers(0, 2, (batch, n), dtype=np.uint8)
        elif kind == LIMB:
            rows[:, e:e + n, :8] = rng.integers(0, 256, (batch, n, 8), dtype=np.uint8)
            pick = rng.integers(0, 4, (batch, n))
            rows[:, e:e + n, :8][pick == 0] = 0
            rows[:, e:e + n, :8][pick == 1] = 255
        else:
            rows[:, e:e + n] = rng.integers(0, 256, (batch, n, 32), dtype=np.uint8)
            pick = rng.integers(0, 8, (batch, n))
            for k in range(4):
                rows[:, e:e + n][pick == k] = fe[k]
        e += n
    return rows
