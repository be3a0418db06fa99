// bsvd.h -- the part of the reference's binary dictionary learning API that this build implements,
// with the reference's signatures, so code written against it links: the greedy sparse-coding step,
// the majority-vote dictionary step and the loop that alternates them. Each function hands its
// matrices to bic::default_device() (bic_gpu.h), which runs the step in the HIP kernels behind bic.h
// and copies the results back; a failing device call prints its reason and aborts, as med() does.
//
// The model is X = A D + E over GF(2): X (n x m) holds one sample per row, D (p x m) one atom per
// row, A (n x p) says which atoms a sample uses and E (n x m) is what they leave unexplained.
// m and p are limited to 1 .. 4096 here. The caller fills D and A; the reference's model
// initialisers, its role-switching learners and its model-order searches are not part of this build
// (DESIGN.md lists them).
#ifndef BSVD_H
#define BSVD_H

#include "binmat.h"

// For every row of E: take the atom nearest to it (the first such atom in D's order) while doing
// so lowers the row's weight, toggling that atom's coefficient in A each time. E and A are updated
// in place. Returns the number of rows that changed.
idx_t update_coefficients_basic(binary_matrix& E, const binary_matrix& D, binary_matrix& A);

// The same step; the reference spreads the rows over OpenMP threads, here both names run the same
// device kernel and give the same result.
idx_t update_coefficients_omp(binary_matrix& E, const binary_matrix& D, binary_matrix& A);

// For every atom, in D's order: a bit of the atom becomes 1 where more than half (integer half) of
// the samples that use the atom want it once the atom is taken out of their residual, else 0. D and
// the residual rows of those samples are updated in place. Returns the number of atoms that changed.
idx_t update_dictionary_steepest(binary_matrix& E, binary_matrix& D, binary_matrix& A);

// The second dictionary rule, a rank-one refinement: for every atom, in D's order, rounds of two halves until
// a round changes nothing. First the atom is voted as above; then every sample (not only the atom's users)
// takes or drops the atom according to whether more than half (integer half) of the atom's set bits are set
// in its residual once the atom is taken out of it. E, D and A are updated in place. Returns the number of
// atoms whose bits changed (an atom whose users alone changed is not counted, as in the reference).
idx_t update_dictionary_proximus(binary_matrix& E, binary_matrix& D, binary_matrix& A);

// The same step; both names run the same device kernels and give the same result.
idx_t update_dictionary_proximus_omp(binary_matrix& E, binary_matrix& D, binary_matrix& A);

// Sets E = A D + X and then alternates the two steps above until neither changes anything.
// Returns the number of iterations run.
idx_t learn_model_traditional(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);

#endif
