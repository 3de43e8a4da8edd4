// ba_se3.hpp -- SE(3) logarithm and inverse left Jacobian in the [omega, upsilon] tangent of the solver's pose update T <- exp(d) T
// (DESIGN.md section 7c): shared by the pose priors and the relative-pose edges (ba_factor.hip).
#pragma once

#include "ba_kernels.hpp"
#include "ba_device.hpp"

namespace cubahip
{

__device__ __forceinline__ void hat3(const Scalar v[3], Scalar M[3][3])
{
	M[0][0] = 0;     M[0][1] = -v[2]; M[0][2] = v[1];
	M[1][0] = v[2];  M[1][1] = 0;     M[1][2] = -v[0];
	M[2][0] = -v[1]; M[2][1] = v[0];  M[2][2] = 0;
}

__device__ __forceinline__ void mul3(const Scalar A[3][3], const Scalar B[3][3], Scalar C[3][3])
{
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) C[i][j] = A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j];
}

// Residual r = [w ; V(w)^-1 (t - R Rbar^T tbar)], w = log(R Rbar^T), of pose (q, t) against (qb, tb) (both unit quaternions), and A = J_w^-1
// = I - W / 2 + d W^2.  The rotation part comes from the relative quaternion (atan2: well defined up to theta = pi).
__device__ __forceinline__ void prior_residual(const Scalar q[4], const Scalar t[3], const Scalar qb[4], const Scalar tb[3], Scalar r[6], Scalar A[3][3])
{
	// qr = q (x) conj(qb)
	Scalar qr[4];
	qr[3] = q[3] * qb[3] + q[0] * qb[0] + q[1] * qb[1] + q[2] * qb[2];
	qr[0] = qb[3] * q[0] - q[3] * qb[0] - (q[1] * qb[2] - q[2] * qb[1]);
	qr[1] = qb[3] * q[1] - q[3] * qb[1] - (q[2] * qb[0] - q[0] * qb[2]);
	qr[2] = qb[3] * q[2] - q[3] * qb[2] - (q[0] * qb[1] - q[1] * qb[0]);
	Scalar inv = 1 / sqrt(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
	if (qr[3] < 0) inv = -inv;
#pragma unroll
	for (int k = 0; k < 4; k++) qr[k] *= inv;
	const Scalar n = sqrt(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2]);
	const Scalar s = n < Scalar(1e-4) ? 2 / qr[3] * (1 - (n / qr[3]) * (n / qr[3]) / 3) : 2 * atan2(n, qr[3]) / n;
	const Scalar w[3] = { s * qr[0], s * qr[1], s * qr[2] };
	Scalar u[3];
	quat_rotate(qr, tb, u);
	u[0] = t[0] - u[0]; u[1] = t[1] - u[1]; u[2] = t[2] - u[2];
	const Scalar th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
	Scalar d;
	if (th < Scalar(0.25)) d = Scalar(1) / 12 + th2 * (Scalar(1) / 720 + th2 * (Scalar(1) / 30240 + th2 * (Scalar(1) / 1209600)));
	else d = (1 - Scalar(0.5) * th * cos(Scalar(0.5) * th) / sin(Scalar(0.5) * th)) / th2;
	Scalar W[3][3], W2[3][3];
	hat3(w, W);
	mul3(W, W, W2);
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) A[i][j] = (i == j ? Scalar(1) : Scalar(0)) - Scalar(0.5) * W[i][j] + d * W2[i][j];
#pragma unroll
	for (int i = 0; i < 3; i++) { r[i] = w[i]; r[3 + i] = A[i][0] * u[0] + A[i][1] * u[1] + A[i][2] * u[2]; }
}

// B = -A Q A, Q = Q(w, v) the lower-left block of the SE(3) left Jacobian in [omega, upsilon] order:
//   Q = P/2 + c1 (WP + PW + WPW) + c2 (WWP + PWW - 3 WPW) + c3 (WPWW + WWPW),  P = [v]x,
//   c1 = (th - sin th) / th^3, c2 = (th^2/2 + cos th - 1) / th^4, c3 = (c2 + 3 (th - sin th - th^3/6) / th^5) / 2 (series below th = 0.25)
__device__ __forceinline__ void prior_jacobian_b(const Scalar r[6], const Scalar A[3][3], Scalar B[3][3])
{
	const Scalar th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], th = sqrt(th2);
	Scalar c1, c2, c3;
	if (th < Scalar(0.25))
	{
		c1 = Scalar(1) / 6 - th2 * (Scalar(1) / 120 - th2 * (Scalar(1) / 5040 - th2 * (Scalar(1) / 362880)));
		c2 = Scalar(1) / 24 - th2 * (Scalar(1) / 720 - th2 * (Scalar(1) / 40320 - th2 * (Scalar(1) / 3628800)));
		c3 = Scalar(1) / 120 - th2 * (Scalar(1) / 2520 - th2 * (Scalar(1) / 120960 - th2 * (Scalar(1) / 9979200)));
	}
	else
	{
		const Scalar sn = sin(th), cs = cos(th), th3 = th2 * th;
		c1 = (th - sn) / th3;
		c2 = (th2 / 2 + cs - 1) / (th2 * th2);
		c3 = Scalar(0.5) * (c2 + 3 * (th - sn - th3 / 6) / (th3 * th2));
	}
	Scalar W[3][3], P[3][3], WP[3][3], PW[3][3], WPW[3][3], Q[3][3];
	hat3(r, W);
	hat3(r + 3, P);
	mul3(W, P, WP);
	mul3(P, W, PW);
	mul3(WP, W, WPW);
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++)
		{
			const Scalar wwp = W[i][0] * WP[0][j] + W[i][1] * WP[1][j] + W[i][2] * WP[2][j];
			const Scalar pww = PW[i][0] * W[0][j] + PW[i][1] * W[1][j] + PW[i][2] * W[2][j];
			const Scalar wpww = WPW[i][0] * W[0][j] + WPW[i][1] * W[1][j] + WPW[i][2] * W[2][j];
			const Scalar wwpw = W[i][0] * WPW[0][j] + W[i][1] * WPW[1][j] + W[i][2] * WPW[2][j];
			Q[i][j] = Scalar(0.5) * P[i][j] + c1 * (WP[i][j] + PW[i][j] + WPW[i][j]) + c2 * (wwp + pww - 3 * WPW[i][j]) + c3 * (wpww + wwpw);
		}
	Scalar QA[3][3];
	mul3(Q, A, QA);
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) B[i][j] = -(A[i][0] * QA[0][j] + A[i][1] * QA[1][j] + A[i][2] * QA[2][j]);
}

}  // namespace cubahip
