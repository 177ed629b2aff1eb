// The rule of AUTH with `digest` identities (tree_auth.hip) in plain C++, like
// zk_aclperm.h: the host compiler builds the very text the kernels run
// (tools/auth_host.cpp puts it under ASan + UBSan on a machine without a GPU).
//   auth_frame            the parse of an AUTH request body (opcode 100):
//                         be32 xid, be32 100, be32 authType, ustring scheme,
//                         buffer auth, and nothing behind it
//   auth_sha1             SHA-1 of a message of at most AUTH_MAX bytes (one
//                         64-byte block up to 55 bytes, two above)
//   auth_b64              base64 of the 20 hash bytes, '=' padded: 28 bytes
//   auth_identity         ZooKeeper's DigestAuthenticationProvider
//                         .generateDigest: user ':' base64(SHA1(credentials)),
//                         user the bytes before the first ':' (all of them if
//                         there is none)
//   auth_match            is an ACL entry's id one stored identity?
//   aclperm_permits_auth  aclperm_permits with one more branch: a `digest`
//                         entry that carries the bit grants when its id is one
//                         of the connection's identities
// The identity table (ZkAuthTable): AUTH_K records a row, each AUTH_REC bytes:
// the id's length as a native int32, then up to AUTH_ID_MAX id bytes.
// Every read of a frame, a message, an id or a record is inside the lengths
// given, whatever they hold; every loop is bounded by them.
#pragma once
#include "zk_aclperm.h"

#if defined(__HIPCC__)
#define ZK_UNROLL _Pragma("unroll")
#else
#define ZK_UNROLL
#endif

namespace zk {

constexpr int32_t ERR_AUTH_FAILED = -115;

constexpr int32_t AUTH_MAX = 119;          // 119 + 1 + 8 = two SHA-1 blocks
constexpr int32_t AUTH_B64 = 28;           // base64 of 20 bytes
constexpr int32_t AUTH_ID_MAX = AUTH_MAX + 1 + AUTH_B64;            // 148
constexpr int32_t AUTH_K = 4;              // identities a connection
constexpr int32_t AUTH_REC = (4 + AUTH_ID_MAX + 15) & ~15;          // 160
constexpr int32_t AUTH_ROW = AUTH_K * AUTH_REC;

// auth_frame's verdicts
enum : int32_t { AF_OK = 0, AF_MALFORMED = 1, AF_SCHEME = 2, AF_LONG = 3 };

struct AuthFrame {
  int32_t status, xid, type, n;   // n: the credentials' length
  int64_t off;                    // where they start, absolute in buf
};

// Frame body [base, base + L) of buf, an AUTH request -> its credentials.
// A negative length reads as empty; the frame ends exactly behind `auth`.
// AF_OK only for the scheme `digest` and at most AUTH_MAX bytes.
ZK_HD AuthFrame auth_frame(const uint8_t* __restrict__ buf, int64_t base,
                           int64_t L) {
  AuthFrame f{AF_MALFORMED, 0, 0, 0, -1};
  if (L < 8) return f;
  const uint8_t* p = buf + base;
  f.xid = ld_be32(p);
  if (ld_be32(p + 4) != OP_AUTH || L < 20) return f;
  f.type = ld_be32(p + 8);
  int64_t sl = ld_be32(p + 12);
  if (sl < 0) sl = 0;
  int64_t k = 16;
  if (sl > L - k) return f;
  const uint8_t* scheme = p + k;
  k += sl;
  if (k + 4 > L) return f;
  int64_t al = ld_be32(p + k);
  k += 4;
  if (al < 0) al = 0;
  if (al != L - k) return f;
  f.off = base + k;
  f.n = (int32_t)(al > AUTH_MAX ? AUTH_MAX + 1 : al);
  f.status = !aclperm_is(scheme, sl, "digest", 6) ? AF_SCHEME
             : al > AUTH_MAX ? AF_LONG : AF_OK;
  return f;
}

ZK_HD uint32_t auth_rol(uint32_t x, int s) {
  return (x << s) | (x >> (32 - s));
}

// Byte j of the padded message: the message, 0x80, zeros, and in the last
// eight bytes of the last block the length in bits (n <= 119: two bytes).
ZK_HD uint32_t auth_pad_byte(const uint8_t* __restrict__ msg, int32_t n,
                             int32_t j, int32_t end) {
  if (j < n) return msg[j];
  if (j == n) return 0x80u;
  if (j == end - 2) return ((uint32_t)n * 8u) >> 8;
  if (j == end - 1) return ((uint32_t)n * 8u) & 255u;
  return 0u;
}

// One block of SHA-1 over a rolling 16-word window; every index into w is a
// constant once the loops are unrolled, so on the device w lives in registers.
ZK_HD void auth_sha1_block(uint32_t (&h)[5], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
  ZK_UNROLL
  for (int t = 0; t < 80; ++t) {
    if (t >= 16) {
      w[t & 15] = auth_rol(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^
                           w[(t + 2) & 15] ^ w[t & 15], 1);
    }
    uint32_t f, k;
    if (t < 20)      { f = (b & c) | (~b & d);          k = 0x5A827999u; }
    else if (t < 40) { f = b ^ c ^ d;                   k = 0x6ED9EBA1u; }
    else if (t < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8F1BBCDCu; }
    else             { f = b ^ c ^ d;                   k = 0xCA62C1D6u; }
    const uint32_t x = auth_rol(a, 5) + f + e + k + w[t & 15];
    e = d;
    d = c;
    c = auth_rol(b, 30);
    b = a;
    a = x;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}

// SHA-1 of msg[0, n), n <= AUTH_MAX (a longer message is cut there) -> the
// five hash words.
ZK_HD void auth_sha1_words(const uint8_t* __restrict__ msg, int32_t n,
                           uint32_t (&h)[5]) {
  if (n < 0) n = 0;
  if (n > AUTH_MAX) n = AUTH_MAX;
  h[0] = 0x67452301u; h[1] = 0xEFCDAB89u; h[2] = 0x98BADCFEu;
  h[3] = 0x10325476u; h[4] = 0xC3D2E1F0u;
  const int32_t nb = n > 55 ? 2 : 1;
  for (int32_t blk = 0; blk < nb; ++blk) {
    uint32_t w[16];
    ZK_UNROLL
    for (int t = 0; t < 16; ++t) {
      const int32_t j = 64 * blk + 4 * t;
      w[t] = (auth_pad_byte(msg, n, j, 64 * nb) << 24) |
             (auth_pad_byte(msg, n, j + 1, 64 * nb) << 16) |
             (auth_pad_byte(msg, n, j + 2, 64 * nb) << 8) |
             auth_pad_byte(msg, n, j + 3, 64 * nb);
    }
    auth_sha1_block(h, w);
  }
}

ZK_HD void auth_sha1(const uint8_t* __restrict__ msg, int32_t n,
                     uint8_t* __restrict__ out20) {
  uint32_t h[5];
  auth_sha1_words(msg, n, h);
  ZK_UNROLL
  for (int k = 0; k < 20; ++k)
    out20[k] = (uint8_t)(h[k >> 2] >> (24 - 8 * (k & 3)));
}

ZK_HD uint8_t auth_b64_char(uint32_t v) {
  v &= 63u;
  return (uint8_t)(v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26)
                   : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/');
}

// Standard base64 of 20 bytes: six groups of three, then two bytes as three
// characters and one '='.
ZK_HD void auth_b64(const uint8_t* __restrict__ in20,
                    uint8_t* __restrict__ out28) {
  ZK_UNROLL
  for (int g = 0; g < 7; ++g) {
    const uint32_t x = ((uint32_t)in20[3 * g] << 16) |
                       ((uint32_t)in20[3 * g + 1] << 8) |
                       (g < 6 ? (uint32_t)in20[3 * g + 2] : 0u);
    out28[4 * g] = auth_b64_char(x >> 18);
    out28[4 * g + 1] = auth_b64_char(x >> 12);
    out28[4 * g + 2] = auth_b64_char(x >> 6);
    out28[4 * g + 3] = g < 6 ? auth_b64_char(x) : (uint8_t)'=';
  }
}

// base64(SHA1(auth[0, n))) -> b64[28]
ZK_HD void auth_digest(const uint8_t* __restrict__ auth, int32_t n,
                       uint8_t (&b64)[AUTH_B64]) {
  uint8_t h20[20];
  auth_sha1(auth, n, h20);
  auth_b64(h20, b64);
}

// The user of credentials auth[0, n): the length of what stands before the
// first ':' (n: there is none).
ZK_HD int32_t auth_user_len(const uint8_t* __restrict__ auth, int32_t n) {
  int32_t u = 0;
  while (u < n && auth[u] != ':') ++u;
  return u;
}

// user ':' b64 -> id[0, ul + 1 + 28)
ZK_HD void auth_identity_put(const uint8_t* __restrict__ auth, int32_t ul,
                             const uint8_t (&b64)[AUTH_B64],
                             uint8_t* __restrict__ id) {
  for (int32_t k = 0; k < ul; ++k) id[k] = auth[k];
  id[ul] = ':';
  ZK_UNROLL
  for (int k = 0; k < AUTH_B64; ++k) id[ul + 1 + k] = b64[k];
}

// Is user ':' b64 the identity record rec (AUTH_REC bytes) holds?
ZK_HD bool auth_identity_is(const uint8_t* __restrict__ auth, int32_t ul,
                            const uint8_t (&b64)[AUTH_B64],
                            const uint8_t* __restrict__ rec) {
  int32_t rl;
  __builtin_memcpy(&rl, rec, 4);
  if (rl != ul + 1 + AUTH_B64 || rl > AUTH_ID_MAX) return false;
  const uint8_t* id = rec + 4;
  bool same = id[ul] == ':';
  ZK_UNROLL
  for (int k = 0; k < AUTH_B64; ++k) same = same && id[ul + 1 + k] == b64[k];
  for (int32_t k = 0; same && k < ul; ++k) same = id[k] == auth[k];
  return same;
}

// The identity of credentials auth[0, n), n <= AUTH_MAX (a longer one is cut
// there) -> id[0, idlen), idlen <= AUTH_ID_MAX.
ZK_HD void auth_identity(const uint8_t* __restrict__ auth, int32_t n,
                         uint8_t* __restrict__ id, int32_t& idlen) {
  if (n < 0) n = 0;
  if (n > AUTH_MAX) n = AUTH_MAX;
  uint8_t b64[AUTH_B64];
  auth_digest(auth, n, b64);
  const int32_t ul = auth_user_len(auth, n);
  auth_identity_put(auth, ul, b64, id);
  idlen = ul + 1 + AUTH_B64;
}

// Is the id [id, id + il) of an ACL entry the identity record rec holds?
// Length first, then bytes; a record whose length is none an identity has
// matches nothing.
ZK_HD bool auth_match(const uint8_t* __restrict__ id, int64_t il,
                      const uint8_t* __restrict__ rec) {
  int32_t rl;
  __builtin_memcpy(&rl, rec, 4);
  if (rl < 1 + AUTH_B64 || rl > AUTH_ID_MAX || il != rl) return false;
  for (int32_t k = 0; k < rl; ++k)
    if (id[k] != rec[4 + k]) return false;
  return true;
}

// aclperm_permits for a peer at addr that holds the identities of the nids
// records at ids (nids clamped to 0..AUTH_K; ids is not read when it is 0).
// `auth`, `sasl` and every other scheme still match nobody.
ZK_HD bool aclperm_permits_auth(const uint8_t* __restrict__ vec, int64_t len,
                                int32_t perm, uint32_t addr,
                                const uint8_t* __restrict__ ids,
                                int32_t nids) {
  if (nids < 0) nids = 0;
  if (nids > AUTH_K) nids = AUTH_K;
  if (len < 4) return false;
  const int32_t n = ld_be32(vec);
  int64_t k = 4;
  for (int32_t j = 0; j < n; ++j) {
    // (every entry takes 12 bytes or more: the walk ends inside len)
    if (k + 8 > len) return false;
    const int32_t perms = ld_be32(vec + k);
    int64_t sl = ld_be32(vec + k + 4);
    k += 8;
    if (sl < 0) sl = 0;
    if (sl > len - k) return false;
    const uint8_t* scheme = vec + k;
    k += sl;
    if (k + 4 > len) return false;
    int64_t il = ld_be32(vec + k);
    k += 4;
    if (il < 0) il = 0;
    if (il > len - k) return false;
    const uint8_t* id = vec + k;
    k += il;
    if ((perms & perm) == 0) continue;
    if (aclperm_is(scheme, sl, "world", 5)) {
      if (aclperm_is(id, il, "anyone", 6)) return true;
    } else if (aclperm_is(scheme, sl, "ip", 2)) {
      if (aclperm_ip_match(id, il, addr)) return true;
    } else if (nids > 0 && aclperm_is(scheme, sl, "digest", 6)) {
      for (int32_t r = 0; r < nids; ++r)
        if (auth_match(id, il, ids + (int64_t)r * AUTH_REC)) return true;
    }
  }
  return false;
}

}  // namespace zk
