// Test-only host build of eigensolver_amd/csrc/es_bessel_complex.hpp and es_cjet.hpp so that the complex Bessel routines, their
// jets and the primitives of the complex scalar can be checked on the CPU: against scipy.special and against the correctly
// rounded values of tests/golden/bessel_complex_truth.npz (tests/test_hostmath_complex.py).  Not part of the product library.
// z = (re, im); complex arrays are interleaved (re, im) pairs, as NumPy's complex128.
#define ES_HD static inline
#include "../../eigensolver_amd/csrc/es_cjet.hpp"

namespace {
using esb::cz;
inline cz at(const double* z, int i) { return cz(z[2 * i], z[2 * i + 1]); }
inline void put(double* o, int i, cz a) { o[2 * i] = a.re; o[2 * i + 1] = a.im; }

// The CF2 loop of esb::cke01, restated with a counter: *k0 is the header's K_0 bit for bit where the restatement is faithful
// (the test asserts that), the return value the number of passes through the loop body -- the last pass used the indices
// i = passes + 1 of qdiv_int and qdiv_cf2a.  0 on the series side of the branch.
int cf2_passes(cz z, cz* k0) {
  using namespace esb;
  if (cz_abs2(z) <= 4.0) return 0;
  cz b = 2.0 * (1.0 + z), d = 1.0 / b, h = d, delh = d;
  cz q1(0.0), q2(1.0);
  const double a1 = 0.25;
  double c = a1, a = -a1;
  cz q(a1);
  cz s = 1.0 + q * delh;
  int passes = 0;
  for (int i = 2; i < 500; ++i) {
    ++passes;
    a -= 2.0 * (double)(i - 1);
    c = qdiv_int(-a * c, i);
    const cz qnew = (q1 - b * q2) * qdiv_cf2a(1.0, i, a);
    q1 = q2;
    q2 = qnew;
    q = q + c * qnew;
    b = b + 2.0;
    d = 1.0 / (b + a * d);
    delh = (b * d - 1.0) * delh;
    h = h + delh;
    const cz dels = q * delh;
    s = s + dels;
    if (!(cz_abs2(dels) >= 1e-34 * cz_abs2(s))) break;
  }
  *k0 = cz_sqrt((0.5 * kPi) / z) / s;
  return passes;
}
}  // namespace

extern "C" {
void hmc_ke_pair(int n, double re, double im, double* out) {
  esb::cz a, b;
  esb::cke_pair(n, esb::cz(re, im), a, b);
  out[0] = a.re; out[1] = a.im; out[2] = b.re; out[3] = b.im;
}
void hmc_ie_pair_from_k(int n, double re, double im, double* out) {
  esb::cz a, b, i0, i1;
  esb::cke_pair(n, esb::cz(re, im), a, b);
  esb::cie_pair_from_k(n, esb::cz(re, im), a, b, i0, i1);
  out[0] = i0.re; out[1] = i0.im; out[2] = i1.re; out[3] = i1.im;
}

// ---- `count` rows per call: order n[i], argument z[i]; o0, o1 (and d0, d1: the z-derivatives) complex arrays ------------------
void hmc_ke_pair_v(const int* n, const double* z, int count, double* o0, double* o1) {
  for (int i = 0; i < count; ++i) {
    cz a, b;
    esb::cke_pair(n[i], at(z, i), a, b);
    put(o0, i, a); put(o1, i, b);
  }
}
void hmc_ie_pair_from_k_v(const int* n, const double* z, int count, double* o0, double* o1) {
  for (int i = 0; i < count; ++i) {
    cz a, b, i0, i1;
    esb::cke_pair(n[i], at(z, i), a, b);
    esb::cie_pair_from_k(n[i], at(z, i), a, b, i0, i1);
    put(o0, i, i0); put(o1, i, i1);
  }
}
// the CJet<1> forms with z the variable
void hmc_ke_pair_jet_v(const int* n, const double* z, int count, double* o0, double* o1, double* d0, double* d1) {
  for (int i = 0; i < count; ++i) {
    esb::CJet<1> K, K1;
    esb::cke_pair(n[i], esb::cjet_variable<1>(at(z, i), 0), K, K1);
    put(o0, i, K.v); put(o1, i, K1.v); put(d0, i, K.d[0]); put(d1, i, K1.d[0]);
  }
}
void hmc_ie_pair_from_k_jet_v(const int* n, const double* z, int count, double* o0, double* o1, double* d0, double* d1) {
  for (int i = 0; i < count; ++i) {
    const esb::CJet<1> Z = esb::cjet_variable<1>(at(z, i), 0);
    esb::CJet<1> K, K1, I, I1;
    esb::cke_pair(n[i], Z, K, K1);
    esb::cie_pair_from_k(n[i], Z, K, K1, I, I1);
    put(o0, i, I.v); put(o1, i, I1.v); put(d0, i, I.d[0]); put(d1, i, I1.d[0]);
  }
}
// ---- the primitives of the complex scalar ----------------------------------------------------------------------------------------
void hmc_sqrt_v(const double* z, int count, double* o) { for (int i = 0; i < count; ++i) put(o, i, esb::cz_sqrt(at(z, i))); }
void hmc_log_v(const double* z, int count, double* o) { for (int i = 0; i < count; ++i) put(o, i, esb::cz_log(at(z, i))); }
void hmc_exp_v(const double* z, int count, double* o) { for (int i = 0; i < count; ++i) put(o, i, esb::cz_exp(at(z, i))); }
void hmc_div_v(const double* a, const double* b, int count, double* o) {
  for (int i = 0; i < count; ++i) put(o, i, at(a, i) / at(b, i));
}
void hmc_rdiv_v(const double* a, const double* b, int count, double* o) {      // a: real
  for (int i = 0; i < count; ++i) put(o, i, a[i] / at(b, i));
}
// passes through the CF2 loop of cke01 per row (0: the series), and the K_0 of the restated loop (untouched where 0)
void hmc_cf2_passes_v(const double* z, int count, int* passes, double* k0) {
  for (int i = 0; i < count; ++i) {
    cz k(0.0);
    passes[i] = cf2_passes(at(z, i), &k);
    put(k0, i, k);
  }
}
}
