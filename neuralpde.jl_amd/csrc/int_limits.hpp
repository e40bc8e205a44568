// int_limits.hpp — size limits of integral terms, shared by the integral kernels (aux_kernels.hpp) and the host side.  (Not a kernel
// header of the network families: aux_limits.hpp is.)
#pragma once
namespace aux {
constexpr int INT_MAX_NODES = 4;      // integral nodes of one term (k_int_expr)
constexpr int INT_MAX_Q = 64;         // Gauss-Legendre nodes per integral node
constexpr int INT_MAX_C = 24;         // jet channels of the kernel that runs an integral term's site set
}  // namespace aux
