// Test-only host build of eigensolver_amd/csrc/es_bessel_complex.hpp so that the complex Bessel routines can be checked
// against scipy.special on the CPU.  Not part of the product library.  z = (re, im); out: interleaved (re, im) pairs.
#define ES_HD static inline
#include "../../eigensolver_amd/csrc/es_bessel_complex.hpp"
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
}
