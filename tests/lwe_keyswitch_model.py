"""Model of the LWE key switch back to the small key (test helper; contract: include/fhe_hip.h, "LWE key switch back to the small key").

Python integers define everything: ksk_generate (from pyoracle.ctr_rand and pyoracle.gaussian_cdt), keyswitch, lwe_phase.  The numpy forms
below them serve the larger shapes of the GPU tests and are checked equal to the integer forms in test_lwe_keyswitch_model.py: the streams
through a vectorised SplitMix64, the product through uint64 matrix products (directly where bit_length(q) + w + ceil(log2 R) <= 64, on
16-bit pieces recombined as Python integers elsewhere).  Nothing here calls the library under test."""
import numpy as np

DRAW_CDT, DRAW_SIGN, DRAW_UNIFORM = 1, 2, 16
M64 = (1 << 64) - 1


def num_digits(q, w):
    return -(-int(q).bit_length() // w)


def embed(v, q):
    """a small signed integer as a residue: -k -> q - k"""
    return int(v) % q


# ---- the definition, in Python integers -------------------------------------------------------------------------------------------
def uniform_draw(orc, q, seed, g):
    """element g of stream `seed`, one-word modulus: word DRAW_UNIFORM + 4 t masked to bit_length(q), rejected until below q; after 64
    rejections the top bit is cleared"""
    bits = int(q).bit_length()
    mask = (1 << bits) - 1
    for t in range(64):
        v = orc.ctr_rand(seed, g, DRAW_UNIFORM + 4 * t) & mask
        if v < q:
            return v
    return v & (mask >> 1)


def gaussian_draw(orc, cdt, seed, g):
    r = orc.ctr_rand(seed, g, DRAW_CDT)
    mag = sum(1 for c in cdt if r >= c)
    return -mag if orc.ctr_rand(seed, g, DRAW_SIGN) >> 63 else mag


def ksk_noise(orc, n_in, K, sigma, seeds):
    """e_r for r < n_in K, signed integers"""
    cdt = orc.gaussian_cdt(sigma)
    return [gaussian_draw(orc, cdt, seeds[1], r) for r in range(n_in * K)]


def ksk_generate(orc, q, s, z, w, noise_scale, sigma, seeds):
    """rows [R][n_out + 1]: row j K + k = (a_0 .. a_{n_out-1}, b), b = s_j (2^(k w) mod q) + [noise_scale e]_q - sum a_i z_i mod q.
    s: residues of limb 0 of the ring key; z: small signed integers."""
    K, n_out = num_digits(q, w), len(z)
    e = ksk_noise(orc, len(s), K, sigma, seeds)
    rows = []
    for r in range(len(s) * K):
        j, k = divmod(r, K)
        a = [uniform_draw(orc, q, seeds[0], r * n_out + i) for i in range(n_out)]
        b = (int(s[j]) * (pow(2, k * w, q)) + embed(noise_scale * e[r], q) - sum(ai * int(zi) for ai, zi in zip(a, z))) % q
        rows.append(a + [b])
    return rows


def digits(v, K, w):
    return [(int(v) >> (k * w)) & ((1 << w) - 1) for k in range(K)]


def round_to(acc, q, q_out):
    return (acc * q_out + q // 2) // q % q_out


def keyswitch(q, w, rows, lwe, q_out=0):
    """lwe: [batch][n_in + 1] below q -> [batch][n_out + 1]"""
    K = num_digits(q, w)
    n_in = len(rows) // K
    out = []
    for ct in lwe:
        assert len(ct) == n_in + 1
        d = [x for v in ct[:n_in] for x in digits(v, K, w)]
        acc = [sum(dr * int(row[i]) for dr, row in zip(d, rows)) % q for i in range(len(rows[0]))]
        acc[-1] = (acc[-1] + int(ct[n_in])) % q
        out.append([round_to(a, q, q_out) for a in acc] if q_out else acc)
    return out


def lwe_phase(q, sample, key):
    """(b + sum a_i key_i) mod q, centred into (-q/2, q/2]"""
    v = (int(sample[-1]) + sum(int(a) * int(k) for a, k in zip(sample[:-1], key))) % q
    return v - q if v > q // 2 else v


def digit_noise(q, w, lwe_ct, e, noise_scale):
    """noise_scale sum_{j,k} d_{j,k} e_{j K + k} for one input ciphertext: what the key switch adds to the phase"""
    K = num_digits(q, w)
    d = [x for v in lwe_ct[:-1] for x in digits(v, K, w)]
    return noise_scale * sum(dr * er for dr, er in zip(d, e))


# ---- numpy forms ---------------------------------------------------------------------------------------------------------------------
def _sm64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def ctr_rand_np(seed, index, draw):
    """pyoracle.ctr_rand over an array of element indices (uint64 wrap-around arithmetic)"""
    with np.errstate(over="ignore"):
        index = np.asarray(index, dtype=np.uint64)
        base = _sm64(np.uint64(seed & M64) ^ (index * np.uint64(0xD1342543DE82EF95)))
        return _sm64(base + np.uint64(draw))


def ksk_noise_np(orc, n_in, K, sigma, seeds):
    cdt = np.array(orc.gaussian_cdt(sigma), dtype=np.uint64)
    r = np.arange(n_in * K, dtype=np.uint64)
    mag = np.searchsorted(cdt, ctr_rand_np(seeds[1], r, DRAW_CDT), side="right").astype(np.int64)      # #{ j : cdt[j] <= draw }
    neg = (ctr_rand_np(seeds[1], r, DRAW_SIGN) >> np.uint64(63)).astype(bool)
    return np.where(neg, -mag, mag)


def ksk_generate_np(orc, q, s, z, w, noise_scale, sigma, seeds):
    """ksk_generate as a uint64 array [R][n_out + 1]"""
    K, n_out, n_in = num_digits(q, w), len(z), len(s)
    R = n_in * K
    bits = int(q).bit_length()
    mask = np.uint64((1 << bits) - 1)
    g = np.arange(R * n_out, dtype=np.uint64)
    a = ctr_rand_np(seeds[0], g, DRAW_UNIFORM) & mask
    for t in range(1, 64):
        bad = np.flatnonzero(a >= np.uint64(q))
        if not bad.size:
            break
        a[bad] = ctr_rand_np(seeds[0], g[bad], DRAW_UNIFORM + 4 * t) & mask
    a = np.where(a >= np.uint64(q), a & (mask >> np.uint64(1)), a).reshape(R, n_out)
    e = ksk_noise_np(orc, n_in, K, sigma, seeds)
    az = a.astype(object) @ np.array([int(v) for v in z], dtype=object)
    rows = np.empty((R, n_out + 1), dtype=np.uint64)
    rows[:, :n_out] = a
    for r in range(R):
        j, k = divmod(r, K)
        rows[r, n_out] = (int(s[j]) * pow(2, k * w, q) + embed(noise_scale * int(e[r]), q) - int(az[r])) % q
    return rows


def digits_np(lwe, K, w):
    """uint64 [batch][n_in + 1] -> uint64 [batch][n_in K], digit k of coefficient j at j K + k"""
    a = np.asarray(lwe, dtype=np.uint64)[:, :-1]
    sh = (np.arange(K, dtype=np.uint64) * np.uint64(w))
    return ((a[:, :, None] >> sh[None, None, :]) & np.uint64((1 << w) - 1)).reshape(a.shape[0], -1)


def u64_form(q, w, R):
    return int(q).bit_length() + w + max(R - 1, 0).bit_length() <= 64


def keyswitch_np(q, w, rows, lwe, q_out=0):
    """keyswitch on arrays: rows uint64 [R][n_out + 1], lwe uint64 [batch][n_in + 1] -> uint64 [batch][n_out + 1]"""
    rows = np.asarray(rows, dtype=np.uint64)
    lwe = np.asarray(lwe, dtype=np.uint64)
    K = num_digits(q, w)
    D = digits_np(lwe, K, w)
    assert D.shape[1] == rows.shape[0]
    if u64_form(q, w, rows.shape[0]):
        acc = (D @ rows).astype(object) % q                       # the whole sum is below 2^64
    else:
        # 16-bit pieces: a product of pieces is below 2^32, a sum over R <= 2^22 rows below 2^54; recombined as Python integers
        acc = np.zeros((lwe.shape[0], rows.shape[1]), dtype=object)
        for dp in range(2):
            Dp = (D >> np.uint64(16 * dp)) & np.uint64(0xFFFF)
            if not Dp.any():
                continue
            for rp in range(4):
                part = Dp @ ((rows >> np.uint64(16 * rp)) & np.uint64(0xFFFF))
                acc = acc + part.astype(object) * (1 << (16 * (dp + rp)))
        acc = acc % q
    acc[:, -1] = (acc[:, -1] + lwe[:, -1].astype(object)) % q
    if q_out:
        acc = (acc * q_out + q // 2) // q % q_out
    return acc.astype(np.uint64)
