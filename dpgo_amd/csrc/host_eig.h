// The certificates' dense eigen-solvers on the host.  No HIP header, no handle: certify.cpp, blockcert.cpp and
// capi.cpp call them, tests/cpp/test_cert_host.cpp checks them without a GPU.  Eigenvalues and eigenvectors are
// separate outputs; eigenvector c of a k x k problem is Z[c * k .. c * k + k).
#pragma once
#include <vector>

namespace dpgo {

// Eigenpairs of the symmetric tridiagonal T (diag a, off-diagonal e[i] between i and i+1) by the implicit QL method
// (at most 200 sweeps per eigenvalue): w the ascending eigenvalues, Z their eigenvectors.  Z = nullptr: eigenvalues
// only, O(k^2).
void tridiag_eig(std::vector<double> a, std::vector<double> e, std::vector<double>& w, std::vector<double>* Z);

// Unit eigenvector of the tridiagonal T (diag a, off-diagonal e) for its lowest eigenvalue th0 (th1 the next):
// inverse iteration with the shift th0 - delta below the spectrum, so T - shift is positive definite and the
// LDL^T (Thomas) solve needs no pivoting; each solve amplifies the wanted component by (th1 - s) / (th0 - s).
std::vector<double> tridiag_lowest_vector(const std::vector<double>& a, const std::vector<double>& e, double th0,
                                          double th1, double scale);

// Eigenpairs of the dense symmetric m x m matrix A (row-major): Householder reduction to tridiagonal form
// (A = Q T Q^T, Q accumulated) and tridiag_eig on T.  w ascending, Z the eigenvectors of A.
void sym_eig(int m, std::vector<double> A, std::vector<double>& w, std::vector<double>& Z);

// Cyclic Jacobi on the symmetric r x r matrix A (r <= 8): on return A's diagonal holds the eigenvalues (unsorted)
// and column c of V the eigenvector of A[c][c].  Row-cyclic sweeps until no off-diagonal entry moves a diagonal one.
void jacobi_eig(int r, double A[8][8], double V[8][8]);

}  // namespace dpgo
