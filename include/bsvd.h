// bsvd.h -- the part of the reference's binary dictionary learning API that this build implements,
// with the reference's signatures, so code written against it links: four model initialisers, the
// greedy sparse-coding step, the two dictionary steps, the loop that alternates them, the three
// role-switching learners, the model code length and the three MDL searches that choose the number of
// atoms, with learn_model_setup and its name tables. Each function
// hands its matrices to bic::default_device() (bic_gpu.h), which runs the step in the HIP kernels behind
// bic.h and copies the results back; a failing device call prints its reason and aborts, as med() does.
//
// The model is X = A D + E over GF(2): X (n x m) holds one sample per row, D (p x m) one atom per
// row, A (n x p) says which atoms a sample uses and E (n x m) is what they leave unexplained.
// p is limited to 1 .. 4096 here; the steps and the learners take m up to 1048576 (the role-switching
// learners n up to 1048576 as well), the model initialisers m up to 4096, and so do the forward and the full
// search, which initialise. A model is started as the reference's driver does it: E = X,
// initialize_model(E, D, A), then a learner. The reference's initialize_model_graph_grow,
// update_coefficients_fast and update_dictionary_steepest_omp are not part of this build (DESIGN.md lists
// them); learn_model_setup names them and exits when asked for one.
#ifndef BSVD_H
#define BSVD_H

#include "binmat.h"

// The model initialisers: D and A are cleared and then made from the data E, which needs at least one
// row; E's padding bits are ignored. The three that draw share one process-wide generator (GSL's rand48
// sequence), seeded from random_seed at the first draw, so consecutive calls continue one sequence.
//
// neighbor: every atom is the centroid of the rows that share a set bit with a randomly picked non-zero
// row (a bit is set where at least half, integer half, of those rows have it in common with the pick);
// aborts when E has no non-zero row, where the reference would not return. A stays zero.
void initialize_model_neighbor(const binary_matrix& E, binary_matrix& D, binary_matrix& A);
// partition: atom k is the centroid of the rows that have the k-th heaviest column set (column weights as
// the reference's col_weight samples them); atoms past the number of columns stay zero. A stays zero.
void initialize_model_partition(const binary_matrix& E, binary_matrix& D, binary_matrix& A);
// random centroids: every row is assigned to a random atom (its coefficient in A is set) and every atom is
// the majority of its rows, a tie setting the bit and an atom without rows being all ones.
void initialize_model_random_centroids(const binary_matrix& E, binary_matrix& D, binary_matrix& A);
// the same assignment; every atom is the XOR of its rows, an atom without rows zero.
void initialize_model_random_centroids_xor(const binary_matrix& E, binary_matrix& D, binary_matrix& A);

typedef void (*mi_algorithm_t)(const binary_matrix& E, binary_matrix& D, binary_matrix& A);
extern mi_algorithm_t initialize_model;  // initialize_model_neighbor unless assigned
extern long random_seed;                 // 34503498; read once, at the first draw

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

typedef idx_t (*cu_algorithm_t)(binary_matrix& E, const binary_matrix& D, binary_matrix& A);
typedef idx_t (*du_algorithm_t)(binary_matrix& E, binary_matrix& D, binary_matrix& A);
typedef idx_t (*ml_algorithm_t)(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);

// The steps the learners below use. update_coefficients is update_coefficients_omp unless assigned (both
// sparse-coding functions run the same kernel, so the learners do not look at it). update_dictionary chooses
// the learners' dictionary rule: it must be one of the four dictionary functions above, anything else makes a
// learner print a message and abort. The reference initialises update_dictionary with itself, i.e. null, and
// crashes unless learn_model_setup ran; here it is update_dictionary_steepest unless assigned.
extern cu_algorithm_t update_coefficients;
extern du_algorithm_t update_dictionary;

// Sets E = A D + X and then alternates the two steps above until neither changes anything.
// Returns the number of iterations run.
idx_t learn_model_traditional(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);

// The role-switching learners: like the loop above, but they also run the two steps on the transposed model,
// where the atoms are the rows of A transposed (one bit per sample) and D transposed holds the coefficients,
// and transpose back; E, D and A come back with zero padding bits. As the reference has them:
// alter1 runs the direct pair and the transposed pair in every pass and goes on only while the transposed
// dictionary step changes an atom; alter2 runs the direct loop to its end, then the transposed loop, and
// repeats both while anything changed (its second direct loop never runs, and it returns the last transposed
// loop's count); alter3 never recodes: the transposed dictionary step, then the direct one, while the direct
// one changes an atom (the one meant for update_dictionary_proximus).
idx_t learn_model_alter1(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);
idx_t learn_model_alter2(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);
idx_t learn_model_alter3(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);

// The code length of a model in bits, the reference's two-part code: universal_codelength (coding.h) of E as
// one string of rows * cols bits, plus that of every atom (m bits) and of every column of A (n bits). As the
// reference computes it: 32-bit arguments, and the running sums of the atoms' and the columns' lengths
// truncated to an integer after every term. D and A without rows and columns give E's length alone.
idx_t model_codelength(const binary_matrix& E, const binary_matrix& D, const binary_matrix& A);

// The learner the MDL searches below run on every candidate, and the learner a driver calls after
// learn_model_setup; both learn_model_traditional unless assigned. learn_model_inner must be one of the four
// learners above, initialize_model one of the four initialisers and update_dictionary one of the four dictionary
// functions: anything else makes a search print a message and abort.
extern ml_algorithm_t learn_model, learn_model_inner;

// The MDL model-order searches: each returns the best code length it found and leaves that model in E, D and A,
// which are re-allocated to its number of atoms. They print the reference's progress lines on stdout and draw
// from the generator the initialisers share. The text's behaviour is kept as written (bic.h "MDL model order"
// lists what looks like slips):
// forward selection learns the given model, then adds one atom per pass, initialised from the current residual
// with initialize_model, and learns again; a pass is accepted when the length falls below the best one by the
// mean excess of the rejected passes so far; the model keeps growing whether or not a pass was accepted, and
// ten rejected passes in a row end the search. This build stops at 4096 atoms (it then prints and aborts).
idx_t learn_model_mdl_forward_selection(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);
// backward selection learns the given model, then removes one atom per pass: the one whose removal, scored
// on the best model's residual, gives the shortest length; then it learns again, with the same accept rule.
// When removing the last atom is accepted, the result is the empty model: D and A are destroyed, E = X, and
// the returned length is the one before that pass.
idx_t learn_model_mdl_backward_selection(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);
// full search tries 20, 40, .. atoms up to D's rows: per size one initialise-and-learn that is thrown away and
// ten that are measured; the size whose minimum is the smallest wins, and the model left is the last of its
// ten runs. With fewer than 20 rows in D nothing runs: E, D and A stay and 1 << 30 is returned.
idx_t learn_model_mdl_full_search(binary_matrix& X, binary_matrix& E, binary_matrix& D, binary_matrix& A);

// Assigns initialize_model, update_coefficients, update_dictionary, learn_model and learn_model_inner from the
// reference's catalogues and prints its "Using ..." lines: mi 0..4, cu 0..2, du 0..3, lm 0..6 (4, 5, 6: the
// searches above), lmi 0..3. An index out of range prints the reference's message and exits; so does one that
// names a piece this build does not have: mi 4 (initialize_model_graph_grow), cu 2 (update_coefficients_fast),
// du 2 (update_dictionary_steepest_omp).
void learn_model_setup(int mi_algo, int cu_algo, int du_algo, int lm_algo, int lmi_algo);
extern const char* mi_algorithm_names[];
extern const char* cu_algorithm_names[];
extern const char* du_algorithm_names[];
extern const char* lm_algorithm_names[];

#endif
