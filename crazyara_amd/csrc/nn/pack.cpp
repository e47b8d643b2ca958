#include "pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

#include "rise_net.h"

namespace cra {

Folded fold_bn(const NetFile& nf, const std::string& conv, const std::string& bn) {
    const TensorView& w = nf.get(conv + ".weight");
    const int64_t cout = w.shape[0], per = w.numel() / cout;
    Folded f;
    f.w.resize(w.numel());
    f.b.assign(cout, 0.0);
    if (bn.empty()) {
        for (int64_t i = 0; i < w.numel(); ++i) f.w[i] = w.data[i];
        return f;
    }
    const float *g = nf.get(bn + ".weight").data, *be = nf.get(bn + ".bias").data, *m = nf.get(bn + ".running_mean").data,
                *v = nf.get(bn + ".running_var").data;
    for (int64_t co = 0; co < cout; ++co) {
        const double sc = double(g[co]) / std::sqrt(double(v[co]) + kBnEps);
        for (int64_t i = 0; i < per; ++i) f.w[co * per + i] = double(w.data[co * per + i]) * sc;
        f.b[co] = double(be[co]) - double(m[co]) * sc;
    }
    return f;
}

BlockFold fold_block(const NetFile& nf, const std::string& p) {
    return BlockFold{fold_bn(nf, p + ".body.0", p + ".body.1"), fold_bn(nf, p + ".body.3", p + ".body.4"), fold_bn(nf, p + ".body.6", p + ".body.7")};
}

namespace {
void expect_shape(const NetFile& nf, const std::string& name, std::vector<int64_t> shape) {
    if (!nf.has(name)) throw std::runtime_error("transformer block: tensor " + name + " is missing");
    if (nf.get(name).shape != shape) {
        std::string want;
        for (int64_t d : shape) want += (want.empty() ? "" : "x") + std::to_string(d);
        throw std::runtime_error("transformer block: tensor " + name + " has the wrong shape (expected " + want + ")");
    }
}
void expect_bn(const NetFile& nf, const std::string& bn, int64_t c) {
    for (const char* t : {".weight", ".bias", ".running_mean", ".running_var"}) expect_shape(nf, bn + t, {c});
}
// a Linear / 1x1 conv with bias, no BN behind it
Folded load_biased(const NetFile& nf, const std::string& name) {
    Folded f = fold_bn(nf, name, "");
    const TensorView& b = nf.get(name + ".bias");
    for (int64_t i = 0; i < b.numel(); ++i) f.b[i] = b.data[i];
    return f;
}
// merge_pre_bn: y = W BN(x) + b = (W diag(s)) x + (b + W (beta - s mean)), s = gamma / sqrt(var + eps); W is [cout][cin]
void fold_pre_bn(Folded& f, const NetFile& nf, const std::string& bn, int cin) {
    const float *g = nf.get(bn + ".weight").data, *be = nf.get(bn + ".bias").data, *m = nf.get(bn + ".running_mean").data,
                *v = nf.get(bn + ".running_var").data;
    const int cout = int(f.b.size());
    for (int co = 0; co < cout; ++co) {
        double extra = 0.0;
        for (int ci = 0; ci < cin; ++ci) {
            const double sc = double(g[ci]) / std::sqrt(double(v[ci]) + kBnEps);
            extra += f.w[size_t(co) * cin + ci] * (double(be[ci]) - double(m[ci]) * sc);
            f.w[size_t(co) * cin + ci] *= sc;
        }
        f.b[co] += extra;
    }
}
}  // namespace

NtbFold fold_ntb(const NetFile& nf, const std::string& p, int C) {
    NtbFold n;
    n.C = C;
    if (!nf.has(p + ".projection.conv.weight") && !nf.has(p + ".mhca.group_conv3x3.weight") && nf.has(p + ".e_mhsa.q.weight"))
        throw std::runtime_error("transformer block " + p + ": the 'simple' NTB variant (no projection / MHCA branch) is not supported");
    if (nf.has(p + ".e_mhsa.norm.weight") || nf.has(p + ".e_mhsa.norm.running_mean"))
        throw std::runtime_error("transformer block " + p + ": E_MHSA with sr_ratio > 1 (e_mhsa.norm present) is not supported");
    if (!nf.has(p + ".patch_embed.conv.weight")) throw std::runtime_error("transformer block: tensor " + p + ".patch_embed.conv.weight is missing");
    const TensorView& pe = nf.get(p + ".patch_embed.conv.weight");
    if (pe.shape.size() != 4 || pe.shape[1] != C || pe.shape[2] != 1 || pe.shape[3] != 1)
        throw std::runtime_error("transformer block: tensor " + p + ".patch_embed.conv.weight has the wrong shape (expected Dx" + std::to_string(C) + "x1x1)");
    n.D = int(pe.shape[0]);
    n.M = C - n.D;
    if (n.D % 32 != 0 || n.M <= 0 || n.M % 32 != 0)
        throw std::runtime_error("transformer block " + p + ": E_MHSA width " + std::to_string(n.D) + " of " + std::to_string(C) +
                                 " channels is not a head_dim-32 split (both parts must be multiples of 32)");
    const int D = n.D, M = n.M;
    expect_bn(nf, p + ".patch_embed.norm", D);
    expect_bn(nf, p + ".norm1", D);
    for (const char* l : {".e_mhsa.q", ".e_mhsa.k", ".e_mhsa.v", ".e_mhsa.proj"}) {
        expect_shape(nf, p + l + ".weight", {D, D});
        expect_shape(nf, p + l + ".bias", {D});
    }
    expect_shape(nf, p + ".projection.conv.weight", {M, D, 1, 1});
    expect_bn(nf, p + ".projection.norm", M);
    if (!nf.has(p + ".mhca.group_conv3x3.weight")) throw std::runtime_error("transformer block: tensor " + p + ".mhca.group_conv3x3.weight is missing");
    const TensorView& gc = nf.get(p + ".mhca.group_conv3x3.weight");
    if (gc.shape.size() != 4 || gc.shape[0] != M || gc.shape[2] != 3 || gc.shape[3] != 3)
        throw std::runtime_error("transformer block: tensor " + p + ".mhca.group_conv3x3.weight has the wrong shape (expected " + std::to_string(M) + "x32x3x3)");
    if (gc.shape[1] != 32)
        throw std::runtime_error("transformer block " + p + ": head_dim " + std::to_string(gc.shape[1]) + " (MHCA group width) is not supported, only 32");
    expect_bn(nf, p + ".mhca.norm", M);
    expect_shape(nf, p + ".mhca.projection.weight", {M, M, 1, 1});
    expect_bn(nf, p + ".norm2", C);
    if (!nf.has(p + ".mlp.conv1.weight")) throw std::runtime_error("transformer block: tensor " + p + ".mlp.conv1.weight is missing");
    n.H = int(nf.get(p + ".mlp.conv1.weight").shape[0]);
    expect_shape(nf, p + ".mlp.conv1.weight", {n.H, C, 1, 1});
    expect_shape(nf, p + ".mlp.conv1.bias", {n.H});
    expect_shape(nf, p + ".mlp.conv2.weight", {C, n.H, 1, 1});
    expect_shape(nf, p + ".mlp.conv2.bias", {C});
    if (n.H % 32 != 0) throw std::runtime_error("transformer block " + p + ": Mlp hidden width must be a multiple of 32");

    n.patch = fold_bn(nf, p + ".patch_embed.conv", p + ".patch_embed.norm");
    n.qkv.w.reserve(size_t(3) * D * D);
    for (const char* l : {".e_mhsa.q", ".e_mhsa.k", ".e_mhsa.v"}) {
        Folded f = load_biased(nf, p + l);
        fold_pre_bn(f, nf, p + ".norm1", D);
        n.qkv.w.insert(n.qkv.w.end(), f.w.begin(), f.w.end());
        n.qkv.b.insert(n.qkv.b.end(), f.b.begin(), f.b.end());
    }
    n.proj = load_biased(nf, p + ".e_mhsa.proj");
    n.projection = fold_bn(nf, p + ".projection.conv", p + ".projection.norm");
    {   // grouped 3x3 (groups = M / 32) as a dense 3x3 that is zero off the diagonal blocks
        const Folded g = fold_bn(nf, p + ".mhca.group_conv3x3", p + ".mhca.norm");
        n.mhca.w.assign(size_t(M) * M * 9, 0.0);
        n.mhca.b = g.b;
        for (int co = 0; co < M; ++co)
            for (int j = 0; j < 32; ++j)
                for (int t = 0; t < 9; ++t) n.mhca.w[(size_t(co) * M + (co / 32) * 32 + j) * 9 + t] = g.w[(size_t(co) * 32 + j) * 9 + t];
    }
    n.mhca_proj = fold_bn(nf, p + ".mhca.projection", "");
    n.mlp1 = load_biased(nf, p + ".mlp.conv1");
    fold_pre_bn(n.mlp1, nf, p + ".norm2", C);
    n.mlp2 = load_biased(nf, p + ".mlp.conv2");
    const double sq = 64.0;
    n.macs = sq * C * D + sq * D * 3.0 * D + 2.0 * sq * 64.0 * D + sq * D * D + sq * D * M + sq * M * 32.0 * 9 + sq * M * M + 2.0 * sq * C * n.H;
    return n;
}

// float -> OCP e4m3fn byte: round to nearest even, subnormals down to 2^-9, beyond +-448 clamps (the device conversion runs with
// MODE.FP16_OVFL = 1 and does the same)
uint8_t to_e4m3(double v) {
    const uint8_t sign = std::signbit(v) ? 0x80 : 0;
    double a = std::fabs(v);
    if (!(a == a)) return uint8_t(sign | 0x7f);
    if (a >= 448.0) return uint8_t(sign | 0x7e);
    if (a < std::ldexp(1.0, -10)) return sign;                   // below half the smallest subnormal (a tie at 2^-10 rounds to even = 0)
    int e;
    (void)std::frexp(a, &e);                                     // a = m * 2^e, m in [0.5, 1)
    int ex = e - 1;                                              // a = (1 + f) * 2^ex
    if (ex < -6) ex = -6;                                        // subnormal range: fixed quantum 2^-9
    const double q = std::ldexp(1.0, ex - 3);                    // spacing of representable values around a
    double n = std::nearbyint(a / q);                            // default rounding mode: nearest even
    int mant = int(n);                                           // in units of q: normal numbers 8..16, subnormals 0..8
    if (ex == -6 && mant < 8) return uint8_t(sign | mant);
    if (mant == 16) { mant = 8; ++ex; }
    if (ex > 8 || (ex == 8 && mant - 8 > 6)) return uint8_t(sign | 0x7e);
    return uint8_t(sign | ((ex + 7) << 3) | (mant - 8));
}
// power of two that brings max |w| of a row into [1, 2); 1 for an all-zero row
double row_scale_pow2(double max_abs) {
    if (!(max_abs > 0.0)) return 1.0;
    int e;
    (void)std::frexp(max_abs, &e);
    e -= 1;
    if (e < -24) e = -24;
    return std::ldexp(1.0, e);
}

// e5m2 ("bf8": f16's exponent field, two mantissa bits), round to nearest even from the float value, subnormals kept, saturating
uint8_t to_e5m2(float f) {
    const uint8_t sign = std::signbit(f) ? 0x80 : 0;
    const double a = std::fabs(double(f));
    if (!(a > 0.0)) return sign;
    int e = 0;
    (void)std::frexp(a, &e);
    int E = e - 1;                                                      // a = 1.m * 2^E
    if (E < -14) {                                                      // subnormal: units of 2^-16
        const int q = int(std::nearbyint(std::ldexp(a, 16)));
        return uint8_t(sign | (q >= 4 ? 0x04 : q));
    }
    int mant = int(std::nearbyint((std::ldexp(a, -E) - 1.0) * 4.0));
    if (mant == 4) { mant = 0; ++E; }
    if (E > 15) return uint8_t(sign | 0x7B);                            // the largest finite value (1.75 * 2^15)
    return uint8_t(sign | ((E + 15) << 2) | mant);
}

uint8_t float_to_e4m3(float v) { return to_e4m3(double(v)); }
uint8_t float_to_e5m2(float v) { return to_e5m2(v); }

template <typename T> std::vector<T> pack_dense(const Folded& f, int cout, int cin, int ks, int cout_pad, int cin_pad) {
    const int kt = ks * ks * cin_pad, nslab = kt / 32, nct = cout_pad / 16;
    std::vector<T> out(size_t(cout_pad) * kt);
    for (int ct = 0; ct < nct; ++ct)
        for (int s = 0; s < nslab; ++s)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int co = ct * 16 + (l & 15);
                    const int k = s * 32 + (l >> 4) * 8 + j;
                    const int tap = k / cin_pad, ci = k % cin_pad;
                    double v = 0.0;
                    if (co < cout && ci < cin) v = f.w[(size_t(co) * cin + ci) * ks * ks + tap];
                    out[((size_t(ct) * nslab + s) * 64 + l) * 8 + j] = T(float(v));
                }
    return out;
}
template std::vector<half_t> pack_dense<half_t>(const Folded&, int, int, int, int, int);
template std::vector<float> pack_dense<float>(const Folded&, int, int, int, int, int);

SplitPack pack_dense_split(const Folded& f, int cout, int cin, int ks, int cout_pad, int cin_pad) {
    Folded fh = f, fl = f;
    for (size_t i = 0; i < f.w.size(); ++i) {
        const half_t h = half_t(float(f.w[i]));
        fh.w[i] = double(float(h));
        fl.w[i] = f.w[i] - fh.w[i];
    }
    return SplitPack{pack_dense<half_t>(fh, cout, cin, ks, cout_pad, cin_pad), pack_dense<half_t>(fl, cout, cin, ks, cout_pad, cin_pad)};
}

// Precision float16p8, expand / project weights of a tower block (x3.hip: tower_p8_kernel; kernels.h: X3TowerBlock; oracle: _p8_conv).
// W' = w * 2^p with p = 11 - floor(log2(max |w|)) (the largest weight lands in [2048, 4096)): hi = rne_f16(W') is the main term's operand;
// the 8-bit image holds, per cout tile and 64 k, a lane's 32 bytes -- lane groups 0, 1: e5m2((W' - hi) * c) for k [0, 32), [32, 64) (they
// meet the activations' hi8), groups 2, 3: e5m2(hi * c) for the same k (they meet the activations' lo8) -- bytes 0-15 in "slab" 2 J, bytes
// 16-31 in "slab" 2 J + 1 of the lo image's geometry.  c = 1 / (1 - ln 2 / 8): the kernel's activation bytes are TRUNCATED f16 values (their
// high bytes), which lose 2^e / 8 on average; the weight images take the mean back.  All three products carry the factor 2^p; *inv = 2^-p.
constexpr double kP8TruncCompensation = 1.0 / (1.0 - 0.125 * 0.6931471805599453);
SplitPack pack_dense_p8(const Folded& f, int cout, int cin, int ks, int cout_pad, int cin_pad, double* inv) {
    double mx = 0.0;
    for (double v : f.w) mx = std::max(mx, std::fabs(v));
    int e = 0;
    if (mx > 0.0) { (void)std::frexp(mx, &e); e -= 1; }               // mx = m * 2^e, m in [1, 2)
    const int p = 11 - e;
    *inv = std::ldexp(1.0, -p);
    Folded fs = f;
    for (double& v : fs.w) v = std::ldexp(v, p);
    SplitPack out;
    out.hi = pack_dense<half_t>(fs, cout, cin, ks, cout_pad, cin_pad);
    const int nslab = ks * ks * cin_pad / 32, nct = cout_pad / 16;     // k = tap * cin_pad + ci, as pack_dense walks it
    if (cin_pad % 64 != 0) throw std::runtime_error("float16p8: K per tap must be a multiple of 64");
    std::vector<uint8_t> bytes(size_t(cout_pad) * ks * ks * cin_pad * 2, 0);
    for (int ct = 0; ct < nct; ++ct)
        for (int J = 0; J < nslab / 2; ++J)
            for (int l = 0; l < 64; ++l)
                for (int bb = 0; bb < 32; ++bb) {
                    const int co = ct * 16 + (l & 15), lg = l >> 4, k = 64 * J + (lg & 1) * 32 + bb;
                    const int tap = k / cin_pad, ci = k % cin_pad;
                    uint8_t q = 0;
                    if (co < cout && ci < cin) {
                        const double W = fs.w[(size_t(co) * cin + ci) * ks * ks + tap];
                        const double hi = double(float(half_t(float(W))));
                        q = to_e5m2(float((lg < 2 ? W - hi : hi) * kP8TruncCompensation));
                    }
                    bytes[((size_t(ct) * nslab + 2 * J + (bb >> 4)) * 64 + l) * 16 + (bb & 15)] = q;
                }
    out.lo.resize(bytes.size() / 2);
    std::memcpy(out.lo.data(), bytes.data(), bytes.size());
    return out;
}

std::vector<float> pack_depthwise_taps(const Folded& dw, int cop, int k, int ld) {
    std::vector<float> w(size_t(k) * k * ld, 0.f);
    for (int c = 0; c < cop; ++c) for (int t = 0; t < k * k; ++t) w[size_t(t) * ld + c] = float(dw.w[size_t(c) * k * k + t]);
    return w;
}

std::vector<float> pack_depthwise_records12(const Folded& bn1, const Folded& dw, int cop, int cop_pad) {
    std::vector<float> rec(size_t(cop_pad) * 12, 0.f);
    for (int c = 0; c < cop; ++c) {
        for (int t = 0; t < 9; ++t) rec[size_t(c) * 12 + t] = float(dw.w[size_t(c) * 9 + t]);
        rec[size_t(c) * 12 + 9] = float(bn1.b[c]);
        rec[size_t(c) * 12 + 10] = float(dw.b[c]);
    }
    return rec;
}

// Precision float16x3, depthwise records of a block.  3x3 (x3.hip: X3Depthwise): per tile of 16 expanded channels 16 rows of 16 floats (1 KiB,
// one 16-byte load per lane) -- rows 0-2 the folded taps of column dx = -1 (dy = -1, 0, 1), rows 3-5 dx = 0, rows 6-8 dx = +1, row 9 the BN1
// bias, row 10 the BN2 bias, rows 11-15 zeros: a lane on file a / h reads its dx = -1 / +1 weights from rows 11-13.  5x5 (X3Depthwise5): per
// tile 32 rows of 16 floats (2 KiB) -- rows 5 g + i the folded taps of column dx = g - 2 (dy = i - 2), row 25 the BN1 bias, row 26 the BN2
// bias, rows 27-31 zeros
std::vector<float> pack_x3_depthwise_records(const Folded& bn1, const Folded& dw, int cop, int cop_pad, int k) {
    const int rows = k == 3 ? 16 : 32;
    std::vector<float> rec(size_t(cop_pad) * rows, 0.f);
    for (int c = 0; c < cop; ++c) {
        float* tile = rec.data() + size_t(c / 16) * rows * 16 + (c % 16);
        for (int dy = 0; dy < k; ++dy)
            for (int dx = 0; dx < k; ++dx) tile[(dx * k + dy) * 16] = float(dw.w[size_t(c) * k * k + dy * k + dx]);
        tile[k * k * 16] = float(bn1.b[c]);
        tile[(k * k + 1) * 16] = float(dw.b[c]);
    }
    return rec;
}

StemStreams pack_stem(const Folded& fs, int cin, int cin_pad16) {
    const int nks = cin_pad16 / 16;
    StemStreams out;
    for (int wv = 0; wv < 8; ++wv) {
        for (int tap = 0; tap < 9; ++tap)
            for (int ksx = 0; ksx < nks; ++ksx)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int co = wv * 32 + (l & 31), ci = ksx * 16 + (l >> 5) * 8 + j;
                        out.w.push_back(half_t(ci < cin ? float(fs.w[(size_t(co) * cin + ci) * 9 + tap]) : 0.f));
                    }
        out.w.insert(out.w.end(), size_t(16) * 512, half_t(0.f));
        for (int lh = 0; lh < 2; ++lh)
            for (int v = 0; v < 16; ++v) out.b.push_back(float(fs.b[wv * 32 + (v % 4) + 8 * (v / 4) + 4 * lh]));
    }
    return out;
}

ResTowerStreams pack_restower(const std::vector<Folded>& f1s, const std::vector<Folded>& f2s, int C, int NR) {
    const int n_waves = 8 / NR;
    ResTowerStreams out;
    for (int wv = 0; wv < n_waves; ++wv) {
        for (size_t i = 0; i < f1s.size(); ++i) {
            for (int cv2 = 0; cv2 < 2; ++cv2) {
                const Folded& fd = cv2 ? f2s[i] : f1s[i];
                for (int tap = 0; tap < 9; ++tap)
                    for (int ksx = 0; ksx < 16; ++ksx)
                        for (int rt = 0; rt < NR; ++rt)
                            for (int l = 0; l < 64; ++l)
                                for (int j = 0; j < 8; ++j) {
                                    const int co = (wv * NR + rt) * 32 + (l & 31), kpos = ksx * 16 + (l >> 5) * 8 + j;
                                    const int ci = cv2 ? (kpos / 32) * 32 + tower_row_of_position(kpos % 32) : kpos;
                                    out.w.push_back(half_t(float(fd.w[(size_t(co) * C + ci) * 9 + tap])));
                                }
                for (int rt = 0; rt < NR; ++rt)
                    for (int lh = 0; lh < 2; ++lh)
                        for (int v = 0; v < 16; ++v) out.b.push_back(float(fd.b[(wv * NR + rt) * 32 + (v % 4) + 8 * (v / 4) + 4 * lh]));
            }
        }
        out.w.insert(out.w.end(), size_t(16) * 512, half_t(0.f));
    }
    return out;
}

void TowerStreams::append(const TowerStreams& o) {
    for (int i = 0; i < 4; ++i) {
        w[i].insert(w[i].end(), o.w[i].begin(), o.w[i].end());
        b[i].insert(b[i].end(), o.b[i].begin(), o.b[i].end());
        p[i].insert(p[i].end(), o.p[i].begin(), o.p[i].end());
        w8e[i].insert(w8e[i].end(), o.w8e[i].begin(), o.w8e[i].end());
        w8p[i].insert(w8p[i].end(), o.w8p[i].begin(), o.w8p[i].end());
    }
}

TowerBlockPack pack_tower_block(const BlockFold& bf, int C, int cop, int k, int q, std::pair<float, float> calib) {
    const Folded &f1 = bf.expand, &f2 = bf.dw;
    Folded f3 = bf.project;
    const bool int8 = q == 2;
    const int cop_pad = round_up(cop, 128), n = cop_pad / 128;
    TowerBlockPack out;
    // Precision fp8: power-of-two scale per expand channel / per cout; s1 goes into the depthwise weights (ReLU commutes with
    // a positive factor), b1 / s1 is where the expand accumulator starts, y = x + s3 * (acc + b3 / s3)
    // Precision int8 (oracle/rise_oracle.py: int8_block is the definition): s1 / s3 = max |row| / 127, weights rounded half to
    // even; with the block's calibrated activation steps 1 / qx_inv (stream) and 1 / qt_inv (depthwise output) a unit of the
    // expand accumulator is worth k1 = s1 / qx_inv, of the project accumulator k3 = s3 / qt_inv: the biases enter the
    // accumulators as round(b / k), t1 = relu(acc) * 2^-7, k1 * 2^7 goes into the depthwise weights, y = x + k3 * acc.
    // A row whose weights are zero (or nothing) beside its bias -- BatchNorm gamma = 0 with a bias, a constant channel -- would get a
    // unit that the bias does not fit: the unit is then taken from the bias (2^14 units in the expand accumulator: t1 = 128, an f16
    // integer; 2^24 in the project accumulator) and the row's weight bytes round to what is left of them in that unit.
    std::vector<double> s1(size_t(cop_pad), 1.0), s3(size_t(C), 1.0);
    std::vector<double> k1(size_t(cop_pad), 1.0), k3(size_t(C), 1.0);
    constexpr double kInt8Escale = 1.0 / 128.0;
    double qx_inv = 0.0, qt_inv = 0.0;
    if (int8) {
        qx_inv = double(float(half_t(float(127.0 / std::max(double(calib.first), 1e-6)))));     // f16 numbers: the kernel's quantiser multiplies in f16
        qt_inv = double(float(half_t(float(255.0 / std::max(double(calib.second), 1e-6)))));
        out.qx_inv = float(qx_inv);
        out.qt_inv = float(qt_inv);
        out.escale = float(kInt8Escale);
    }
    auto weight_byte = [&](double v) -> uint8_t {               // v = w / row step
        if (!int8) return to_e4m3(v);
        const double r = std::max(-127.0, std::min(127.0, std::nearbyint(v)));
        return uint8_t(int8_t(int(r)));
    };
    if (q != 0) {
        for (int ch = 0; ch < cop; ++ch) {
            double m = 0;
            for (int k2 = 0; k2 < C; ++k2) m = std::max(m, std::fabs(f1.w[size_t(ch) * C + k2]));
            s1[ch] = int8 ? std::max(m, 1e-30) / 127.0 : row_scale_pow2(m);
            k1[ch] = s1[ch] / qx_inv;
            if (std::fabs(f1.b[ch]) > k1[ch] * 4194304.0) {                 // round(b / k1) * 2^-7 would leave the f16 range of t1
                k1[ch] = std::fabs(f1.b[ch]) / 16384.0;
                s1[ch] = k1[ch] * qx_inv;
            }
        }
        for (int co = 0; co < C; ++co) {
            double m = 0;
            for (int ch = 0; ch < cop; ++ch) m = std::max(m, std::fabs(f3.w[size_t(co) * cop + ch]));
            s3[co] = int8 ? std::max(m, 1e-30) / 127.0 : row_scale_pow2(m);
            k3[co] = s3[co] / qt_inv;
            if (std::fabs(f3.b[co]) > k3[co] * 1073741824.0) {              // round(b / k3) would leave the int32 accumulator
                k3[co] = std::fabs(f3.b[co]) / 16777216.0;
                s3[co] = k3[co] * qt_inv;
            }
        }
        for (int w = 0; w < 4; ++w)
            for (int c = 0; c < n; ++c) {
                for (int ks = 0; ks < 4; ++ks)           // expand: [k-step of 64][half][lane][16 B]
                    for (int hf = 0; hf < 2; ++hf)
                        for (int l = 0; l < 64; ++l)
                            for (int t = 0; t < 16; ++t) {
                                const int ch = c * 128 + w * 32 + (l & 31), k2 = ks * 64 + (l >> 5) * 32 + hf * 16 + t;
                                out.s.w8e[w].push_back(ch < cop ? weight_byte(f1.w[size_t(ch) * C + k2] / s1[ch]) : uint8_t(0));
                            }
                for (int ks = 0; ks < 2; ++ks)           // project: [k-step of 64][row tile][half][lane][16 B]
                    for (int rt = 0; rt < 2; ++rt)
                        for (int hf = 0; hf < 2; ++hf)
                            for (int l = 0; l < 64; ++l)
                                for (int t = 0; t < 16; ++t) {
                                    const int co = w * 64 + rt * 32 + (l & 31);
                                    const int ch = tower_k_channel(c * 128 + ks * 64 + (l >> 5) * 32 + hf * 16 + t);
                                    out.s.w8p[w].push_back(ch < cop ? weight_byte(f3.w[size_t(co) * cop + ch] / s3[co]) : uint8_t(0));
                                }
            }
        if (int8) {
            // project accumulators: int32, started at round(b3 / k3) + 128 x the row's weight sum (the depthwise output u is held as
            // u - 128); y = x + k3 * acc.  The bit patterns travel in the float arrays the fp8 path uses.
            out.b3.resize(size_t(C));
            out.s3.resize(size_t(C));
            for (int co = 0; co < C; ++co) {
                long long rowsum = 0;
                for (int ch = 0; ch < cop; ++ch) rowsum += (long long)(int8_t(weight_byte(f3.w[size_t(co) * cop + ch] / s3[co])));
                const int32_t start = int32_t(std::nearbyint(f3.b[co] / k3[co])) + int32_t(128 * rowsum);
                std::memcpy(&out.b3[co], &start, 4);
                out.s3[co] = float(k3[co]);
            }
        } else {
            for (int co = 0; co < C; ++co) f3.b[co] /= s3[co];
            out.s3.assign(s3.begin(), s3.end());
        }
    }
    if (!int8) out.b3.assign(f3.b.begin(), f3.b.end());
    for (int w = 0; w < 4; ++w) {
        std::vector<half_t>& ws = out.s.w[w];
        for (int kk = -1; kk <= n && q == 0; ++kk) {      // interval: E(kk+1) then P(kk-1); the 8-bit modes read w8e / w8p instead
            if (kk + 1 < n) {                              // expand A fragments [k-step]: rows = my 32 channels, k = input channel
                const int c = kk + 1;
                for (int ks = 0; ks < 16; ++ks)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int ch = c * 128 + w * 32 + (l & 31), k = ks * 16 + (l >> 5) * 8 + j;
                            ws.push_back(half_t(ch < cop ? float(f1.w[size_t(ch) * C + k]) : 0.f));
                        }
            }
            if (kk - 1 >= 0) {                             // project A fragments [k-step][row tile]: rows = my 64 couts, k = tower K position
                const int c = kk - 1;
                for (int ks = 0; ks < 8; ++ks)
                    for (int rt = 0; rt < 2; ++rt)
                        for (int l = 0; l < 64; ++l)
                            for (int j = 0; j < 8; ++j) {
                                const int co = w * 64 + rt * 32 + (l & 31);
                                const int ch = tower_k_channel(c * 128 + ks * 16 + (l >> 5) * 8 + j);
                                ws.push_back(half_t(ch < cop ? float(f3.w[size_t(co) * cop + ch]) : 0.f));
                            }
            }
        }
        for (int c = 0; c < n; ++c) {
            for (int lh = 0; lh < 2; ++lh)                  // BN1 biases [lane/32][accumulator element v]
                for (int v = 0; v < 16; ++v) {
                    const int ch = c * 128 + w * 32 + (v % 4) + 8 * (v / 4) + 4 * lh;
                    if (int8) {                             // int32 bit pattern of the BN1 bias in the accumulator's unit
                        const int32_t start = ch < cop ? int32_t(std::nearbyint(f1.b[ch] / k1[ch])) : 0;
                        float bits;
                        std::memcpy(&bits, &start, 4);
                        out.s.b[w].push_back(bits);
                    } else
                        out.s.b[w].push_back(ch < cop ? float(f1.b[ch] / s1[ch]) : 0.f);
                }
            // depthwise weights for K positions w*32 + lg*8 + pi*2 + {0,1}, entries = k*k taps then the BN2 bias:
            //   5 x 5: [32 entries][lg][pair pi][2]   (entry-major: the four lane groups of a broadcast read sit in four bank slots)
            //   3 x 3: [10 entries][lg][file variant][pair pi][2], variant 0 = file a (taps with dx = -1 zeroed), 1 = files b..g,
            //          2 = file h (dx = +1 zeroed); zero padding up to the chunk's 2 KiB
            auto dwv = [&](int lgk, int ent, int pi, int hh) {
                const int ch = tower_k_channel(c * 128 + w * 32 + lgk * 8 + pi * 2 + hh);
                double v = 0.0;
                if (ch < cop && ent <= k * k) v = ent < k * k ? f2.w[size_t(ch) * k * k + ent] * (int8 ? k1[ch] / kInt8Escale : s1[ch]) : f2.b[ch];
                return v;
            };
            std::vector<half_t>& ps = out.s.p[w];
            const size_t chunk_begin = ps.size();
            if (k == 3) {
                for (int ent = 0; ent < 10; ++ent)
                    for (int lgk = 0; lgk < 4; ++lgk)
                        for (int var = 0; var < 3; ++var)
                            for (int pi = 0; pi < 4; ++pi)
                                for (int hh = 0; hh < 2; ++hh) {
                                    const bool off_board = ent < 9 && ((var == 0 && ent % 3 == 0) || (var == 2 && ent % 3 == 2));
                                    ps.push_back(half_t(off_board ? 0.f : float(dwv(lgk, ent, pi, hh))));
                                }
            } else {
                for (int ent = 0; ent < 32; ++ent)
                    for (int lgk = 0; lgk < 4; ++lgk)
                        for (int pi = 0; pi < 4; ++pi)
                            for (int hh = 0; hh < 2; ++hh) ps.push_back(half_t(float(dwv(lgk, ent, pi, hh))));
            }
            ps.resize(chunk_begin + 1024, half_t(0.f));
        }
    }
    return out;
}

TowerImage close_tower_streams(TowerStreams r, bool fp8) {
    TowerImage out;
    if (fp8) {
        for (int w = 0; w < 4; ++w) {        // [expand stream + a window of zeros][project stream + a window of zeros]
            r.w8e[w].resize(r.w8e[w].size() + 8 * 1024, 0);
            r.w8p[w].resize(r.w8p[w].size() + 8 * 1024, 0);
            out.w8.insert(out.w8.end(), r.w8e[w].begin(), r.w8e[w].end());
            out.w8.insert(out.w8.end(), r.w8p[w].begin(), r.w8p[w].end());
        }
        out.e_frags = (long long)(r.w8e[0].size() / 1024);
    }
    for (int w = 0; w < 4; ++w) {
        r.w[w].resize(r.w[w].size() + size_t(kTowerWindow) * 512, half_t(0.f));
        r.p[w].resize(r.p[w].size() + 1024, half_t(0.f));
        r.b[w].resize(r.b[w].size() + 32, 0.f);
        out.w.insert(out.w.end(), r.w[w].begin(), r.w[w].end());
        out.b.insert(out.b.end(), r.b[w].begin(), r.b[w].end());
        out.p.insert(out.p.end(), r.p[w].begin(), r.p[w].end());
    }
    out.w_wave_frags = fp8 ? (long long)((r.w8e[0].size() + r.w8p[0].size()) / 1024) : (long long)(r.w[0].size() / 512);
    out.b_wave_floats = (long long)r.b[0].size();
    out.p_wave_bytes = (long long)(r.p[0].size() * sizeof(half_t));
    return out;
}

X3NtbPack pack_x3_ntb(const NtbFold& n) {
    const int C = n.C, D = n.D, M = n.M, H = n.H;
    if (D % 32 != 0 || M % 32 != 0 || H % 32 != 0 || C != D + M) throw std::runtime_error("pack_x3_ntb: widths must be multiples of 32");
    X3NtbPack out;
    out.patch = pack_dense_split(n.patch, D, C, 1, D, C);
    out.qkv = pack_dense_split(n.qkv, 3 * D, D, 1, 3 * D, D);
    out.proj = pack_dense_split(n.proj, D, D, 1, D, D);
    out.projection = pack_dense_split(n.projection, M, D, 1, M, D);
    Folded g;                                                 // the diagonal blocks of fold_ntb's dense image: [M][32][3][3]
    g.b = n.mhca.b;
    g.w.resize(size_t(M) * 32 * 9);
    for (int co = 0; co < M; ++co)
        for (int j = 0; j < 32; ++j)
            for (int t = 0; t < 9; ++t) g.w[(size_t(co) * 32 + j) * 9 + t] = n.mhca.w[(size_t(co) * M + (co / 32) * 32 + j) * 9 + t];
    out.mhca = pack_dense_split(g, M, 32, 3, M, 32);
    out.mhca_proj = pack_dense_split(n.mhca_proj, M, M, 1, M, M);
    out.mlp1 = pack_dense_split(n.mlp1, H, C, 1, H, C);
    out.mlp2 = pack_dense_split(n.mlp2, C, H, 1, C, H);
    return out;
}

X3BlockPack pack_x3_block(const BlockFold& bf, int C, int cop, int k, int cop_pad, bool p8) {
    X3BlockPack out;
    out.w1 = p8 ? pack_dense_p8(bf.expand, cop, C, 1, cop_pad, C, &out.w1_inv) : pack_dense_split(bf.expand, cop, C, 1, cop_pad, C);
    out.w3 = p8 ? pack_dense_p8(bf.project, C, cop, 1, C, cop_pad, &out.w3_inv) : pack_dense_split(bf.project, C, cop, 1, C, cop_pad);
    out.dw = pack_x3_depthwise_records(bf.expand, bf.dw, cop, cop_pad, k);
    out.b3.assign(bf.project.b.begin(), bf.project.b.end());
    return out;
}

SEWeights load_se(const NetFile& nf, const std::string& p, const std::string& type, int C) {
    SEWeights se;
    if (type == "ca_se" || type == "se") {           // _ChannelAttentionModule, builder_util.py:83-114
        const TensorView &w1 = nf.get(p + ".se.fc.0.weight"), &w2 = nf.get(p + ".se.fc.2.weight");
        const int H = C / 2;
        se.w0.resize(size_t(C) * H);
        se.w1.resize(size_t(H) * C);
        for (int j = 0; j < H; ++j) for (int c = 0; c < C; ++c) se.w0[size_t(c) * H + j] = w1.data[size_t(j) * C + c];
        for (int c = 0; c < C; ++c) for (int j = 0; j < H; ++j) se.w1[size_t(j) * C + c] = w2.data[size_t(c) * H + j];
        se.kind = 1;
        se.macs = 2.0 * C * H;
    } else if (type == "eca_se") {                   // _EfficientChannelAttentionModule, builder_util.py:49-80
        const TensorView& w = nf.get(p + ".se.body.0.weight");     // [C][C][kk]; the length-1 sequence only sees the centre tap
        const int kk = int(w.shape[2]), mid = kk / 2;
        se.w0.resize(size_t(C) * C);
        for (int o = 0; o < C; ++o) for (int c = 0; c < C; ++c) se.w0[size_t(c) * C + o] = w.data[(size_t(o) * C + c) * kk + mid];
        const float* bs = nf.get(p + ".se.body.0.bias").data;
        se.b.assign(bs, bs + C);
        se.kind = 2;
        se.macs = double(C) * C;
    } else if (type != "none" && !type.empty()) {
        throw std::runtime_error("unsupported se_type " + type);
    }
    return se;
}

// tower kernel, SE gate weights in thread order: thread t of 512 reads its 32 half2 weights as 8 coalesced 16-byte loads,
// load i of thread t at uint4 index i*512 + t (tower.hip: se_phase).  idx(t, k) = half2 index of thread t's k-th weight.
template <typename Idx> static std::vector<half_t> pack_se_threads(const std::vector<float>& src, Idx idx) {
    std::vector<half_t> out(size_t(8) * 512 * 8);
    for (int i = 0; i < 8; ++i)
        for (int t = 0; t < 512; ++t)
            for (int j = 0; j < 4; ++j) {
                const size_t h2 = idx(t, 4 * i + j);
                out[((size_t(i) * 512 + t) * 4 + j) * 2 + 0] = half_t(src[2 * h2]);
                out[((size_t(i) * 512 + t) * 4 + j) * 2 + 1] = half_t(src[2 * h2 + 1]);
            }
    return out;
}

std::pair<std::vector<half_t>, std::vector<half_t>> pack_se_tower(const SEWeights& se) {
    if (se.kind == 1)
        // FC1: thread t -> outputs 2*(t/8), +1 over inputs c in [32*(t%8), +32); FC2: outputs 2*(t/4), +1 over j in [32*(t%4), +32):
        // the threads of an output pair are neighbouring lanes (in-wave reduction, tower.hip: se_phase)
        return {pack_se_threads(se.w0, [](int t, int k) { return size_t((t & 7) * 32 + k) * 64 + (t >> 3); }),
                pack_se_threads(se.w1, [](int t, int k) { return size_t((t & 3) * 32 + k) * 128 + (t >> 2); })};
    // eca_se: thread t -> outputs 2*(t/4), +1 over inputs i in [64*(t%4), +64): first 32 inputs, then the second 32
    std::vector<half_t> pk = pack_se_threads(se.w0, [](int t, int k) { return size_t((t & 3) * 64 + k) * 128 + (t >> 2); });
    const std::vector<half_t> pk2 = pack_se_threads(se.w0, [](int t, int k) { return size_t((t & 3) * 64 + 32 + k) * 128 + (t >> 2); });
    pk.insert(pk.end(), pk2.begin(), pk2.end());
    return {pk, {}};
}

// the float16x3 tower's gate matrices in thread order (x3.hip: x3_se_phase): thread t of 512 reads 16 float4, load i at float4 index
// i * 512 + t = (a[2i], b[2i], a[2i+1], b[2i+1]) of its two output rows a, b; w(row, k) returns the matrix entry for the thread's k-th input
template <typename W> static std::vector<float> pack_se_threads_f32(W w) {
    std::vector<float> out(size_t(16) * 512 * 4);
    for (int i = 0; i < 16; ++i)
        for (int t = 0; t < 512; ++t)
            for (int e = 0; e < 4; ++e) out[(size_t(i) * 512 + t) * 4 + e] = w(t, e & 1, 2 * i + (e >> 1));
    return out;
}

std::pair<std::vector<float>, std::vector<float>> pack_se_x3(const SEWeights& se, int C) {
    const std::vector<float>& w = se.w0;
    if (se.kind == 1) {
        const int H = C / 2;
        // FC1: thread t -> hidden rows 2*(t/8), +1 over inputs c = 32*(t%8) + k;  FC2: gate rows 2*(t/4), +1 over hidden j = 32*(t%4) + k
        return {pack_se_threads_f32([&](int t, int row, int k) { return w[size_t(32 * (t & 7) + k) * H + 2 * (t >> 3) + row]; }),
                pack_se_threads_f32([&](int t, int row, int k) { return se.w1[size_t(32 * (t & 3) + k) * C + 2 * (t >> 2) + row]; })};
    }
    // eca_se: thread t -> gate rows 2*(t/4), +1 over inputs i = 64*(t%4) + k: the first 32 inputs, then (second image) the other 32
    std::vector<float> pk = pack_se_threads_f32([&](int t, int row, int k) { return w[size_t(64 * (t & 3) + k) * C + 2 * (t >> 2) + row]; });
    const std::vector<float> pk2 = pack_se_threads_f32([&](int t, int row, int k) { return w[size_t(64 * (t & 3) + 32 + k) * C + 2 * (t >> 2) + row]; });
    pk.insert(pk.end(), pk2.begin(), pk2.end());
    return {pk, {}};
}

HeadStreams pack_head(const Folded& f1, const Folded& f2, const Folded& fv, int C, int cv, int cp) {
    HeadStreams out;
    const half_t hz = half_t(0.f);
    for (int wv = 0; wv < 8; ++wv) {
        for (int tap = 0; tap < 9; ++tap)
            for (int ks = 0; ks < 16; ++ks)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int co = wv * 32 + (l & 31), ci = ks * 16 + (l >> 5) * 8 + j;
                        out.s1.push_back(half_t(float(f1.w[(size_t(co) * C + ci) * 9 + tap])));
                    }
        for (int ks = 0; ks < 16; ++ks)          // value head 1x1 conv (wave 0), rows 0..7
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int row = l & 31, ci = ks * 16 + (l >> 5) * 8 + j;
                    out.s1.push_back(wv == 0 && row < cv ? half_t(float(fv.w[size_t(row) * C + ci])) : hz);
                }
        out.s1.insert(out.s1.end(), size_t(16) * 512, hz);
        for (int lh = 0; lh < 2; ++lh)
            for (int v = 0; v < 16; ++v) out.b1.push_back(float(f1.b[wv * 32 + (v % 4) + 8 * (v / 4) + 4 * lh]));
        for (int i = 0; i < 18; ++i) {
            const int u = wv * 18 + i, tap = u >> 4, ks = u & 15;
            for (int rt = 0; rt < 3; ++rt)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int co = rt * 32 + (l & 31), kpos = ks * 16 + (l >> 5) * 8 + j;
                        const int ci = (kpos / 32) * 32 + tower_row_of_position(kpos % 32);
                        out.s2.push_back(co < cp ? half_t(float(f2.w[(size_t(co) * C + ci) * 9 + tap])) : hz);
                    }
        }
        out.s2.insert(out.s2.end(), size_t(9) * 512, hz);
    }
    return out;
}

std::vector<float> pack_value_wdl(const NetFile& nf, int nfl, int pitch) {
    const TensorView &ww = nf.get("value_head.body_wdl.0.weight"), &wp = nf.get("value_head.body_plys.0.weight");
    std::vector<float> w4(size_t(4) * pitch, 0.f);
    for (int r = 0; r < 3; ++r) std::copy(ww.data + size_t(r) * nfl, ww.data + size_t(r + 1) * nfl, w4.begin() + size_t(r) * pitch);
    std::copy(wp.data, wp.data + nfl, w4.begin() + size_t(3) * pitch);
    return w4;
}

std::vector<half_t> pack_value_fc1_threads(const NetFile& nf, int nfl, int fc) {
    const TensorView& w1 = nf.get("value_head.body_final.0.weight");
    // thread order (head.hip, phase 4): thread t of 512 owns outputs 2*(t/4), +1 over k in [128*(t%4), +128); its load i is the
    // uint4 at index i*512 + t = the (w[2j2][k], w[2j2+1][k]) pairs of k = 128*(t%4) + 4i .. 4i+3; k >= nfl: zeros
    std::vector<half_t> w1t(size_t(512) * fc, half_t(0.f));
    for (int i = 0; i < 32; ++i)
        for (int t = 0; t < 512; ++t)
            for (int j = 0; j < 4; ++j) {
                const int k = 128 * (t & 3) + 4 * i + j, o = 2 * (t >> 2);
                if (k >= nfl) continue;
                w1t[((size_t(i) * 512 + t) * 4 + j) * 2 + 0] = half_t(w1.data[size_t(o) * nfl + k]);
                w1t[((size_t(i) * 512 + t) * 4 + j) * 2 + 1] = half_t(w1.data[size_t(o + 1) * nfl + k]);
            }
    return w1t;
}

std::vector<float> pack_value_fc1_transposed(const NetFile& nf, int nfl, int fc) {
    const TensorView& w1 = nf.get("value_head.body_final.0.weight");
    std::vector<float> w1t(size_t(nfl) * fc);
    for (int t = 0; t < fc; ++t) for (int i = 0; i < nfl; ++i) w1t[size_t(i) * fc + t] = w1.data[size_t(t) * nfl + i];
    return w1t;
}

}  // namespace cra
