// ndt_host.h — the host-side pre- and post-steps that CRegistration::omp_ndt and omp_gicp have in common (ndt.cpp defines them, gicp.cpp calls them):
// the argument checks of a problem, Eigen's isIdentity of the guess, the packed upload of a cloud and T = T_reg * guess
#pragma once
#include <string>

#include "ctx.h"

namespace ndt_host
{
bool cloud_on_device(mulls_ctx *ctx, const mulls_cloud &c);
bool is_identity(const double *G, double prec); // Eigen's isIdentity(prec) of a column-major 4 x 4
int check_problem(const mulls_ndt_problem &P, std::string &msg);
int upload_cloud(mulls_ctx *ctx, const mulls_cloud &c, unsigned char *dst, unsigned char *pinned);
void pose_times_guess(const double *Tn, const double *G, double *T);
} // namespace ndt_host
