// coding.cpp -- include/coding.h (reference: coding.cpp:19-32).
#include "coding.h"

#include "bic.h"

double enumerative_codelength(const unsigned n, const unsigned r) { return bic_enum_codelength(n, r); }

// (the formula lives behind the C ABI, where bic_bsvd_model_codelength evaluates it too)
double universal_codelength(const unsigned n, const unsigned r) { return bic_universal_codelength(n, r); }
