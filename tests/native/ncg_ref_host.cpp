// Host reference of the CorrNMF embedding solves, problem by problem: salamander_amd/csrc/salnmf_ncg_machine.h (the
// Newton-CG every device form runs, as a resumable state machine) driven by an evaluator that forms the objective, the
// gradient and the Hessian-vector product in long double and rounds each result once to double.
//
// Every problem is general: its own term matrix L (T x dim; shared between problems by index), per-term offsets
// off_i (= sample scaling + signature scaling, added in double as the device does), aux_i and start point x0:
//   minimise  -[ sum_i aux_i <L_i, x> - sum_i exp(off_i + <L_i, x>) - |x|^2 / (2 var) ]
// which covers sample solves (terms = signatures), joint multi-modal sample solves (terms = the signatures of every
// modality, off_i = alpha_mod(i) + beta_i), signature solves (terms = samples, L = U) and single problems alike.
//
// Besides the unperturbed run (run 0) it makes n_pert perturbed runs (antithetic pairs: runs 2j+1 and 2j+2 draw the same
// numbers with opposite signs): every evaluation result q gets  delta * scale(q) * xi,  xi uniform in [-1, 1], scale(q)
// the magnitude of the terms q sums (f: |lin| + sum w + |x|^2 / 2var; gradient m: sum |w_i L_im| + |sg_m| + |x_m| / var;
// Hessian-vector product m: sum |hw_i s_i L_im| + |p_m| / var).  tests/_ncg_ref.py classifies a problem as stable
// when every run ends alike.  Test infrastructure only: not part of libsalnmf.so.
//
// argv: input file, output file, threads.  Little-endian binary.
//   input:  int32 n_mats, n_probs, n_pert; double delta;
//           per matrix  int32 T, dim; double L[T * dim] (row-major);
//           per problem int32 mat, maxiter (<= 0: 200 dim); double variance, off[T], aux[T], x0[dim]
//   output: per problem, per run (0 .. n_pert): int32 status, rounds, point evaluations; double x[dim]
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../salamander_amd/csrc/salnmf_ncg_machine.h"

namespace {

struct HostVec {
    static constexpr int n = 64;
    double v[n];
    static double reduce(double s) { return s; }
};

struct Mat {
    int T, dim;
    std::vector<double> L;
};

struct Problem {
    int mat, maxiter;
    double variance;
    std::vector<double> off, aux, x0;
};

struct Result {
    int status, rounds, points;
    double x[64];
};

// splitmix64: xi in [-1, 1]
struct Rng {
    uint64_t s;
    double next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        z ^= z >> 31;
        return (double)(z >> 11) * 0x1.0p-52 - 1.0;
    }
};

using ld = long double;

Result solve(const Mat& M, const Problem& P, double delta, uint64_t seed, double sign) {
    using namespace salnmf::ncgm;
    const int T = M.T, dim = M.dim;
    const double* L = M.L.data();
    const ld var = P.variance;
    std::vector<ld> s(T), hw(T), sg(dim, 0.0L);
    for (int i = 0; i < T; ++i)
        for (int m = 0; m < dim; ++m) sg[m] += (ld)P.aux[i] * L[(size_t)i * dim + m];
    Rng rng{seed};
    auto perturb = [&](ld q, ld scale) -> double {
        const double v = (double)q;
        if (delta == 0.0) return v;
        return v + (double)(sign * delta * rng.next() * scale);
    };
    HostVec x0{};
    for (int m = 0; m < dim; ++m) x0.v[m] = P.x0[m];
    Machine<HostVec> mc;
    mc.begin(x0);
    Result res{};
    const int maxiter = P.maxiter > 0 ? P.maxiter : 200 * dim;
    while (!mc.finished()) {
        const int req = mc.request();
        const HostVec& y = req == REQ_HESSP ? mc.ps : mc.yv;
        for (int i = 0; i < T; ++i) {
            ld acc = 0.0L;
            for (int m = 0; m < dim; ++m) acc += (ld)L[(size_t)i * dim + m] * y.v[m];
            s[i] = acc;
        }
        HostVec r{};
        double f = 0.0;
        if (req == REQ_POINT) {
            ld lin = 0.0L, ex = 0.0L, yy = 0.0L;
            for (int i = 0; i < T; ++i) {
                hw[i] = expl((ld)P.off[i] + s[i]);
                lin += s[i] * P.aux[i];
                ex += hw[i];
            }
            for (int m = 0; m < dim; ++m) yy += (ld)y.v[m] * y.v[m];
            f = perturb(-(lin - ex - yy / (2 * var)), fabsl(lin) + ex + yy / (2 * var));
            for (int m = 0; m < dim; ++m) {
                ld comb = 0.0L, mag = 0.0L;
                for (int i = 0; i < T; ++i) {
                    const ld t = hw[i] * L[(size_t)i * dim + m];
                    comb += t;
                    mag += fabsl(t);
                }
                r.v[m] = perturb(-(sg[m] - comb - y.v[m] / var), mag + fabsl(sg[m]) + fabsl((ld)y.v[m]) / var);
            }
            ++res.points;
        } else {
            for (int m = 0; m < dim; ++m) {
                ld comb = 0.0L, mag = 0.0L;
                for (int i = 0; i < T; ++i) {
                    const ld t = hw[i] * s[i] * L[(size_t)i * dim + m];
                    comb += t;
                    mag += fabsl(t);
                }
                r.v[m] = perturb(comb + y.v[m] / var, mag + fabsl((ld)y.v[m]) / var);
            }
        }
        mc.advance(f, r, dim, maxiter);
        ++res.rounds;
    }
    res.status = mc.status;
    for (int m = 0; m < dim; ++m) res.x[m] = mc.xk.v[m];
    return res;
}

template <class X>
bool get(FILE* f, X* p, size_t n) {
    return fread(p, sizeof(X), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hdr[3];
    double delta;
    if (!get(in, hdr, 3) || !get(in, &delta, 1)) return 2;
    const int n_mats = hdr[0], n_probs = hdr[1], n_pert = hdr[2];
    std::vector<Mat> mats(n_mats);
    for (Mat& M : mats) {
        int32_t td[2];
        if (!get(in, td, 2) || td[0] < 1 || td[1] < 1 || td[1] > HostVec::n) return 2;
        M.T = td[0];
        M.dim = td[1];
        M.L.resize((size_t)M.T * M.dim);
        if (!get(in, M.L.data(), M.L.size())) return 2;
    }
    std::vector<Problem> probs(n_probs);
    for (Problem& P : probs) {
        int32_t mi[2];
        if (!get(in, mi, 2) || mi[0] < 0 || mi[0] >= n_mats) return 2;
        P.mat = mi[0];
        P.maxiter = mi[1];
        const Mat& M = mats[P.mat];
        P.off.resize(M.T);
        P.aux.resize(M.T);
        P.x0.resize(M.dim);
        if (!get(in, &P.variance, 1) || !get(in, P.off.data(), M.T) || !get(in, P.aux.data(), M.T) || !get(in, P.x0.data(), M.dim)) return 2;
    }
    fclose(in);
    const int runs = n_pert + 1;
    std::vector<Result> out((size_t)n_probs * runs);
    std::atomic<int64_t> next{0};
    const int64_t n_tasks = (int64_t)n_probs * runs;
    auto worker = [&] {
        for (int64_t t; (t = next.fetch_add(1)) < n_tasks;) {
            const int p = (int)(t / runs), r = (int)(t % runs);
            const double sign = r == 0 ? 0.0 : ((r - 1) % 2 ? -1.0 : 1.0);
            const uint64_t seed = 0x5eed0000ULL + (uint64_t)p * 1000003ULL + (uint64_t)((r + 1) / 2);
            out[t] = solve(mats[probs[p].mat], probs[p], r == 0 ? 0.0 : delta, seed, sign);
        }
    };
    const int n_threads = std::max(1, std::min(atoi(argv[3]), 16));
    std::vector<std::thread> pool;
    for (int i = 0; i < n_threads; ++i) pool.emplace_back(worker);
    for (auto& th : pool) th.join();
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int64_t t = 0; t < n_tasks; ++t) {
        const Result& R = out[t];
        const int dim = mats[probs[t / runs].mat].dim;
        const int32_t head[3] = {R.status, R.rounds, R.points};
        fwrite(head, sizeof(int32_t), 3, o);
        fwrite(R.x, sizeof(double), dim, o);
    }
    return fclose(o) == 0 ? 0 : 2;
}
