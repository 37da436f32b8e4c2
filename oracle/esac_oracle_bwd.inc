/*
 * esac_oracle_bwd.inc -- oracle restatement of esac_backward (code/esac/esac.cpp:213-511) with
 * esac_derivative.h and esac_loss.h.  Included at the end of esac_oracle.c (shares its static helpers).
 * TEST INFRASTRUCTURE ONLY; same parity status as the forward oracle (control flow pinned against the
 * reference sources through oracle/_ref, OpenCV internals restated from memory).
 *
 *   getReproErrs(calcJ=true)   esac_util.h:320-352   -> repro_errs_jac()
 *   loss / calcAngularDistance esac_loss.h:45-83     -> loss_fn()
 *   dLoss                      esac_loss.h:94-210    -> dloss_fn()          (incl. the sqrt(loss) quirk at :133-137)
 *   dProjectdObj               esac_derivative.h:47-102   -> dproject_dobj()
 *   dPNP                       esac_derivative.h:128-185  -> dpnp_p3p()     (float central differences, eps 1e-3f)
 *   dScore / dSMScore          esac_derivative.h:205-420  -> path II below
 *   esac_backward              esac.cpp:213-511      -> esac_oracle_backward()
 */
#define PROB_THRESH_REF 0.001 /* esac_derivative.h:33 */
#define MAXLOSS_REF 10000000.0 /* esac_loss.h:33 */
#define PI_REF 3.1415926       /* esac_util.h:40 (used by calcAngularDistance) */

/* u, v (double) and the two Jacobian rows wrt (rvec, tvec) of one point: cvProjectPoints2 */
static void proj_jac(const double R[9], const double dRdr[27], const double t[3], double fx, double fy, double cx,
                     double cy, double X, double Y, double Z, double* u, double* v, double Ju[6], double Jv[6]) {
    double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    z = z ? 1. / z : 1;
    x *= z;
    y *= z;
    *u = x * fx + cx;
    *v = y * fy + cy;
    Ju[3] = fx * z; Ju[4] = 0;      Ju[5] = -fx * x * z;
    Jv[3] = 0;      Jv[4] = fy * z; Jv[5] = -fy * y * z;
    for (int j = 0; j < 3; j++) {
        const double* dR = dRdr + 9 * j;
        double dx0 = X * dR[0] + Y * dR[1] + Z * dR[2];
        double dy0 = X * dR[3] + Y * dR[4] + Z * dR[5];
        double dz0 = X * dR[6] + Y * dR[7] + Z * dR[8];
        Ju[j] = fx * (z * (dx0 - x * dz0));
        Jv[j] = fy * (z * (dy0 - y * dz0));
    }
}

/* d err / d pose row of one correspondence (esac_util.h:333-351 and esac.cpp:417-431): returns 0 if skipped */
static int norm_jac_row(const double R[9], const double dRdr[27], const double t[3], const ctx_t* c, float X, float Y,
                        float Z, float px, float py, float maxReproj, double row[6]) {
    double u, v, Ju[6], Jv[6];
    proj_jac(R, dRdr, t, c->fx, c->fy, c->cx, c->cy, X, Y, Z, &u, &v, Ju, Jv);
    const float uf = (float)u, vf = (float)v; /* projections are Point2f */
    double err = norm2f(uf - px, vf - py);
    err = err > EPS_REF ? err : EPS_REF; /* std::max(norm, EPS) */
    for (int k = 0; k < 6; k++) row[k] = 0;
    if (err > maxReproj) return 0;
    const double dNdP0 = 1 / err * (uf - px);
    const double dNdP1 = 1 / err * (vf - py);
    for (int k = 0; k < 6; k++) row[k] = dNdP0 * Ju[k] + dNdP1 * Jv[k];
    return 1;
}

/* getReproErrs with calcJ = true: errs (y,x) and J rows indexed ptIdx = x*H + y (push_back order) */
static void repro_errs_jac(const ctx_t* c, const double pose[6], int expert, float* errs, double* J) {
    const esac_oracle_args* a = c->a;
    double R[9], dRdr[27];
    esac_oracle_rodrigues_vec2mat(pose, R, dRdr);
    for (int x = 0; x < a->W; x++)
        for (int y = 0; y < a->H; y++) {
            int px, py;
            px_of(a, x, y, &px, &py);
            const float X = sc_at(a, expert, 0, y, x), Y = sc_at(a, expert, 1, y, x), Z = sc_at(a, expert, 2, y, x);
            float u, v;
            project_point(R, pose + 3, c->fx, c->fy, c->cx, c->cy, X, Y, Z, &u, &v);
            float l = (float)norm2f((float)px - u, (float)py - v);
            errs[y * a->W + x] = a->max_reproj < l ? a->max_reproj : l; /* std::min(l, maxReproj): NaN stays NaN */
            norm_jac_row(R, dRdr, pose + 3, c, X, Y, Z, (float)px, (float)py, a->max_reproj, J + ((size_t)x * a->H + y) * 6);
        }
}

/* pseudo-inverse of a symmetric 6x6 (cv::Mat::inv(DECOMP_SVD)) */
static void pinv_sym6(const double A_in[36], double Ainv[36]) {
    double A[36], w[6], V[36];
    memcpy(A, A_in, sizeof(A));
    jacobi_sym(6, A, w, V);
    double thresh = 0;
    for (int i = 0; i < 6; i++) thresh += fabs(w[i]);
    thresh *= 2 * DBL_EPSILON;
    memset(Ainv, 0, 36 * sizeof(double));
    for (int k = 0; k < 6; k++) {
        if (!(fabs(w[k]) > thresh)) continue;
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) Ainv[i * 6 + j] += V[i * 6 + k] * V[j * 6 + k] / w[k];
    }
}

/* esac_derivative.h:47-102.  f, ppx, ppy are read from the FLOAT camera matrix. */
static void dproject_dobj(float ptx, float pty, float ox, float oy, float oz, const double R[9], const double t[3],
                          const esac_oracle_args* a, float maxReproErr, double out[3]) {
    const double f = (double)a->focal, ppx = (double)a->ppx, ppy = (double)a->ppy;
    out[0] = out[1] = out[2] = 0;
    const double X = R[0] * ox + R[1] * oy + R[2] * oz + t[0];
    const double Y = R[3] * ox + R[4] * oy + R[5] * oz + t[1];
    const double Z = R[6] * ox + R[7] * oy + R[8] * oz + t[2];
    if (fabs(Z) < EPS_REF) return;
    const double px = f * X / Z + ppx;
    const double py = f * Y / Z + ppy;
    double err = sqrt((ptx - px) * (ptx - px) + (pty - py) * (pty - py));
    if (err > maxReproErr) return;
    err += EPS_REF;
    for (int k = 0; k < 3; k++) {
        const double pxd = f * R[0 + k] / Z - f * X / Z / Z * R[6 + k];
        const double pyd = f * R[3 + k] / Z - f * Y / Z / Z * R[6 + k];
        out[k] = 0.5 / err * (2 * (ptx - px) * -pxd + 2 * (pty - py) * -pyd);
    }
}

/* esac_loss.h:45-83 on the 4x4 camera transforms */
static double loss_fn(const double T1[16], const double T2[16], double wRot, double wTrans, double cut) {
    double tr = 0; /* trace(rot2 * rot1^T): each diagonal entry of the product first, then their sum */
    for (int i = 0; i < 3; i++) {
        double d = 0;
        for (int k = 0; k < 3; k++) d += T2[4 * i + k] * T1[4 * i + k];
        tr += d;
    }
    tr = tr < 3.0 ? (tr > -1.0 ? tr : -1.0) : 3.0;
    const double rotErr = 180 * acos((tr - 1.0) / 2.0) / PI_REF;
    double d2 = 0;
    for (int i = 0; i < 3; i++) d2 += (T1[4 * i + 3] - T2[4 * i + 3]) * (T1[4 * i + 3] - T2[4 * i + 3]);
    const double tErr = sqrt(d2);
    double loss = wRot * rotErr + wTrans * tErr;
    if (loss > cut) loss = sqrt(cut * loss);
    return loss < MAXLOSS_REF ? loss : MAXLOSS_REF;
}

/* esac_loss.h:94-210: 1x6 derivative of the loss wrt the estimated scene pose (rvec, tvec) */
static void dloss_fn(const double est[6], const double gt[6], double wRot, double wTrans, double cut, double jac[6]) {
    double R1[9], dRod[27], R2[9];
    esac_oracle_rodrigues_vec2mat(est, R1, dRod);
    esac_oracle_rodrigues_vec2mat(gt, R2, NULL);
    for (int k = 0; k < 6; k++) jac[k] = 0;
    /* diffRot = rot1 * rot2^T */
    double tr = 0;
    for (int a = 0; a < 3; a++) {
        double d = 0;
        for (int cc = 0; cc < 3; cc++) d += R1[3 * a + cc] * R2[3 * a + cc];
        tr += d;
    }
    tr = tr < 3.0 ? (tr > -1.0 ? tr : -1.0) : 3.0;
    const double rotErr = 180 * acos((tr - 1.0) / 2.0) / CV_PI_;
    double invT1[3], invT2[3];
    for (int i = 0; i < 3; i++) {
        invT1[i] = R1[0 + i] * est[3] + R1[3 + i] * est[4] + R1[6 + i] * est[5]; /* rot1^T * t1 */
        invT2[i] = R2[0 + i] * gt[3] + R2[3 + i] * gt[4] + R2[6 + i] * gt[5];
    }
    double d2 = 0;
    for (int i = 0; i < 3; i++) d2 += (invT1[i] - invT2[i]) * (invT1[i] - invT2[i]);
    const double tErr = sqrt(d2);
    double loss = wRot * rotErr + wTrans * tErr;
    int cutLoss = 0;
    if (loss > cut) {
        loss = sqrt(loss); /* sic: sqrt(loss), not sqrt(cut*loss) -- kept bug-compatible */
        cutLoss = 1;
    }
    if (loss > MAXLOSS_REF) return;
    if ((tErr + rotErr) < EPS_REF) return;
    double dD[3];
    for (int i = 0; i < 3; i++) dD[i] = (invT1[i] - invT2[i]) / tErr;
    /* translation part: dDist_dInvT1 (1x3) * invRot1 (3x3), invRot1 = rot1^T */
    for (int j = 0; j < 3; j++) {
        double s = 0;
        for (int i = 0; i < 3; i++) s += dD[i] * R1[3 * j + i];
        jac[3 + j] += s * wTrans;
    }
    /* rotation part through invT1: dDist_dInvT1 (1x3) * dInvT1_dInvRot1 (3x9) * dRod^T (9x3) */
    double g9[9];
    for (int k = 0; k < 9; k++) g9[k] = 0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) g9[3 * j + i] += dD[i] * est[3 + j];
    for (int m = 0; m < 3; m++) {
        double s = 0;
        for (int k = 0; k < 9; k++) s += g9[k] * dRod[9 * m + k];
        jac[m] += s * wTrans;
    }
    /* angular part: dTrace * dRotDiff^T * dRod^T, d diffRot[a][b] / d rot1[a][c] = invRot2[c][b] = rot2[b][c] */
    double h9[9];
    for (int a = 0; a < 3; a++)
        for (int cc = 0; cc < 3; cc++) h9[3 * a + cc] = R2[3 * a + cc];
    const double fac = 180 / CV_PI_ * -1 / sqrt(3 - tr * tr + 2 * tr);
    for (int m = 0; m < 3; m++) {
        double s = 0;
        for (int k = 0; k < 9; k++) s += h9[k] * dRod[9 * m + k];
        jac[m] += fac * s * wRot;
    }
    if (cutLoss)
        for (int k = 0; k < 6; k++) jac[k] *= 0.5 / loss;
    for (int k = 0; k < 6; k++)
        if (jac[k] != jac[k]) {
            for (int q = 0; q < 6; q++) jac[q] = 0;
            return;
        }
}

/* trans2pose (esac_util.h:555-568): inverse, then matrix -> rvec */
static void trans2pose_fn(const double T[16], double pose[6]) {
    double Ti[16], R[9];
    esac_oracle_inv4(T, Ti);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = Ti[4 * i + j];
    esac_oracle_rodrigues_mat2vec_svd(R, pose);
    pose[3] = Ti[3]; pose[4] = Ti[7]; pose[5] = Ti[11];
}

/* dPNP for the 4-point P3P case (esac_derivative.h:128-185): 6x12, last three columns zero */
static int dpnp_p3p(const ctx_t* c, const float img[8], const float obj_in[12], double J[72]) {
    const float eps = 0.001f;
    float obj[12];
    memcpy(obj, obj_in, sizeof(obj));
    memset(J, 0, 72 * sizeof(double));
    double imgd[8];
    for (int k = 0; k < 8; k++) imgd[k] = img[k];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double od[12], f[6], b[6];
            obj[3 * i + j] += eps;
            for (int k = 0; k < 12; k++) od[k] = obj[k];
            if (!esac_oracle_p3p(od, imgd, c->fx, c->fy, c->cx, c->cy, f, f + 3)) { memset(J, 0, 72 * sizeof(double)); return 0; }
            obj[3 * i + j] -= 2 * eps;
            for (int k = 0; k < 12; k++) od[k] = obj[k];
            if (!esac_oracle_p3p(od, imgd, c->fx, c->fy, c->cx, c->cy, b, b + 3)) { memset(J, 0, 72 * sizeof(double)); return 0; }
            obj[3 * i + j] += eps;
            const double den = (double)(2 * eps);
            for (int k = 0; k < 6; k++) {
                const double g = (f[k] - b[k]) / den;
                J[k * 12 + i * 3 + j] = g;
            }
            for (int k = 0; k < 6; k++)
                if (J[k * 12 + i * 3 + j] != J[k * 12 + i * 3 + j]) { memset(J, 0, 72 * sizeof(double)); return 0; }
        }
    return 1; /* (0: a solve failed or an entry is NaN -- the matrix is all zero, esac_derivative.h:150-181) */
}

/* exported for the oracle/_ref shim: (J^T J).inv(DECOMP_SVD) and cv::projectPoints' Jacobian columns 0..5 */
void esac_oracle_pinv_sym6(const double A[36], double Ainv[36]) { pinv_sym6(A, Ainv); }
void esac_oracle_project_jac(const double rvec[3], const double tvec[3], double fx, double fy, double cx, double cy,
                             const float* pts3, int n, double* J12) {
    double R[9], dRdr[27], u, v;
    esac_oracle_rodrigues_vec2mat(rvec, R, dRdr);
    for (int i = 0; i < n; i++)
        proj_jac(R, dRdr, tvec, fx, fy, cx, cy, pts3[3 * i], pts3[3 * i + 1], pts3[3 * i + 2], &u, &v, J12 + 12 * i, J12 + 12 * i + 6);
}

static double get_max_abs(const double* m, size_t n) { /* esac_util.h:599-613 */
    double mx = -1;
    for (size_t i = 0; i < n; i++) {
        const double v = fabs(m[i]);
        if (mx < 0 || v > mx) mx = v;
    }
    return mx;
}

/* Path I, path II and the assembly of esac_backward (esac.cpp:375-508) as a function of GIVEN upstream stages: the second half of
 * esac_oracle_backward, which runs it on its own stages, and -- exported as esac_oracle_backward_paths -- the replay that tests
 * run on another implementation's stages.  errs / JH: the reprojection errors and Jacobian rows of the initial hypotheses
 * (getReproErrs, esac.cpp:295-305), computed here from init_hyps when NULL. */
static void backward_paths(const ctx_t* cp, esac_oracle_bwd_args* b, const esac_oracle_bwd_stages* st_in, const float* errs_in,
                           const double* JH_in, int nthreads) {
    const ctx_t c = *cp;
    const esac_oracle_args* a = c.a;
    const int N = a->N, H = a->H, W = a->W, P = H * W;
    (void)nthreads;
    const double wRot = (double)b->w_rot, wTrans = (double)b->w_trans, cut = (double)b->loss_cut;
    double gtT[16];
    for (int i = 0; i < 16; i++) gtT[i] = (double)b->gt_pose[i];
    const double* initHyps = st_in->init_hyps;
    const double* refHyps = st_in->ref_hyps;
    const int32_t* sxy = st_in->sample_xy;
    const double* probs = st_in->probs;
    const double* losses = st_in->losses;
    const uint8_t* have_map = st_in->have_map;
    const uint8_t* maps = st_in->maps;
    float* errs_own = NULL;
    double* JH_own = NULL;
    if (!errs_in || !JH_in) {
        errs_own = (float*)malloc((size_t)N * P * sizeof(float));
        JH_own = (double*)malloc((size_t)N * P * 6 * sizeof(double));
#pragma omp parallel for schedule(static) num_threads(nthreads)
        for (int h = 0; h < N; h++)
            repro_errs_jac(&c, initHyps + 6 * h, (int)assign_at(a, h), errs_own + (size_t)h * P, JH_own + (size_t)h * P * 6);
    }
    const float* errs = errs_own ? errs_own : errs_in;
    const double* JH = JH_own ? JH_own : JH_in;
    double* gradI = (double*)calloc((size_t)N * P * 3, sizeof(double));   /* gradients[h], 1 x 3P, idx*3+c */
    double* gradII = (double*)calloc((size_t)N * P * 3, sizeof(double));  /* dLoss_dScore_dObjs[h], (y*W+x, c) */
    double* sgrad = (double*)calloc((size_t)N, sizeof(double));
    double* dl_all = (double*)calloc((size_t)N * 6, sizeof(double));
    if (b->out_path1_state) for (int h = 0; h < N; h++) b->out_path1_state[h] = -1;
    if (b->out_dpnp_state) for (int h = 0; h < N; h++) b->out_dpnp_state[h] = -1;
    if (b->out_score_grads) memset(b->out_score_grads, 0, (size_t)N * sizeof(double));

    double hypGT[6];
    trans2pose_fn(gtT, hypGT);
    /* ---- path I: pose -> coordinates through the last re-fit (esac.cpp:375-463) ---- */
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
    for (int h = 0; h < N; h++) {
        if (probs[h] < PROB_THRESH_REF) continue;
        const int expert = (int)assign_at(a, h);
        double* g = gradI + (size_t)h * P * 3;
        double dL[6];
        if (st_in->dloss) memcpy(dL, st_in->dloss + 6 * h, sizeof(dL)); /* a replay: the caller's own dLoss */
        else dloss_fn(refHyps + 6 * h, hypGT, wRot, wTrans, cut, dL);
        memcpy(dl_all + 6 * h, dL, sizeof(dL));
        if (b->out_path1_state) b->out_path1_state[h] = 1;
        if (!have_map[h]) continue;
        /* inliers of the last accepted refinement step, x outer / y inner */
        int n = 0;
        for (int i = 0; i < P; i++) n += maps[(size_t)h * P + i];
        if (b->out_path1_state) b->out_path1_state[h] = 2;
        if (n < 4) continue;
        double* JR = (double*)malloc((size_t)n * 6 * sizeof(double));
        int* cell = (int*)malloc((size_t)n * sizeof(int));
        double R[9], dRdr[27];
        const double* pose = refHyps + 6 * h;
        esac_oracle_rodrigues_vec2mat(pose, R, dRdr);
        int k = 0;
        for (int x = 0; x < W; x++)
            for (int y = 0; y < H; y++)
                if (maps[(size_t)h * P + y * W + x]) {
                    int px, py;
                    px_of(a, x, y, &px, &py);
                    norm_jac_row(R, dRdr, pose + 3, &c, sc_at(a, expert, 0, y, x), sc_at(a, expert, 1, y, x),
                                 sc_at(a, expert, 2, y, x), (float)px, (float)py, a->max_reproj, JR + (size_t)k * 6);
                    cell[k++] = y * W + x;
                }
        /* jacobeanR = -(J^T J).inv(SVD) * J^T   (6 x n) */
        double A[36], Ainv[36];
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) {
                double s = 0;
                for (int q = 0; q < n; q++) s += JR[(size_t)q * 6 + i] * JR[(size_t)q * 6 + j];
                A[i * 6 + j] = s;
            }
        pinv_sym6(A, Ainv);
        if (b->out_jtj) memcpy(b->out_jtj + 36 * (size_t)h, A, sizeof(A));
        double* PI6 = (double*)malloc((size_t)n * 6 * sizeof(double)); /* column q of jacobeanR */
        for (int q = 0; q < n; q++)
            for (int i = 0; i < 6; i++) {
                double s = 0;
                for (int j = 0; j < 6; j++) s += -Ainv[i * 6 + j] * JR[(size_t)q * 6 + j];
                PI6[(size_t)q * 6 + i] = s;
            }
        if (b->out_jr_max) b->out_jr_max[h] = get_max_abs(PI6, (size_t)n * 6);
        if (b->out_path1_state) b->out_path1_state[h] = get_max_abs(PI6, (size_t)n * 6) > 10 ? 3 : 0;
        if (get_max_abs(PI6, (size_t)n * 6) > 10) memset(PI6, 0, (size_t)n * 6 * sizeof(double)); /* clamping for stability */
        for (int q = 0; q < n; q++) {
            const int y = cell[q] / W, x = cell[q] % W;
            int px, py;
            px_of(a, x, y, &px, &py);
            double dNdO[3];
            dproject_dobj((float)px, (float)py, sc_at(a, expert, 0, y, x), sc_at(a, expert, 1, y, x),
                          sc_at(a, expert, 2, y, x), R, pose + 3, a, a->max_reproj, dNdO);
            for (int cc = 0; cc < 3; cc++) {
                double s = 0; /* dLoss_dHyp (1x6) * dHyp_dObjs[:, col] */
                for (int i = 0; i < 6; i++) s += dL[i] * (PI6[(size_t)q * 6 + i] * dNdO[cc]);
                g[(size_t)cell[q] * 3 + cc] = s;
            }
        }
        free(JR); free(cell); free(PI6);
    }

    /* ---- path II: score -> coordinates (dSMScore / dScore, esac_derivative.h:205-420) ---- */
#pragma omp parallel for schedule(static) num_threads(nthreads)
    for (int i = 0; i < N; i++) {
        if (probs[i] < PROB_THRESH_REF) continue;
        double s = probs[i] * losses[i];
        for (int j = 0; j < N; j++) s -= probs[i] * probs[j] * losses[j];
        sgrad[i] = s;
        if (b->out_score_grads) b->out_score_grads[i] = s;
        if (st_in->score_grads) sgrad[i] = st_in->score_grads[i]; /* a replay: the caller's own d E / d score feeds path II */
    }
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
    for (int h = 0; h < N; h++) {
        if (probs[h] < PROB_THRESH_REF) continue;
        const int expert = (int)assign_at(a, h);
        double* g2 = gradII + (size_t)h * P * 3;
        float img[8], obj[12];
        for (int j = 0; j < 4; j++) {
            const int x = sxy[8 * h + 2 * j], y = sxy[8 * h + 2 * j + 1];
            int px, py;
            px_of(a, x, y, &px, &py);
            img[2 * j] = (float)px; img[2 * j + 1] = (float)py;
            for (int k = 0; k < 3; k++) obj[3 * j + k] = sc_at(a, expert, k, y, x);
        }
        double dHdO[72];
        const int solved = dpnp_p3p(&c, img, obj, dHdO);
        if (b->out_dpnp_max) b->out_dpnp_max[h] = get_max_abs(dHdO, 72);
        if (b->out_dpnp_state) b->out_dpnp_state[h] = !solved ? 1 : get_max_abs(dHdO, 72) > 10 ? 2 : 0;
        double dHdO_raw[72], support_raw[12]; /* (out_support_raw only: what the support terms would be WITHOUT the clamp) */
        memcpy(dHdO_raw, dHdO, sizeof(dHdO));
        memset(support_raw, 0, sizeof(support_raw));
        if (get_max_abs(dHdO, 72) > 10) memset(dHdO, 0, sizeof(dHdO));
        if (b->out_dpnp) memcpy(b->out_dpnp + 72 * (size_t)h, dHdO, sizeof(dHdO));
        const double* pose = initHyps + 6 * h;
        double R[9];
        esac_oracle_rodrigues_vec2mat(pose, R, NULL);
        const float scale = a->inlier_alpha / W / H;
        double support[12];
        memset(support, 0, sizeof(support));
        for (int x = 0; x < W; x++)
            for (int y = 0; y < H; y++) {
                double st = a->inlier_beta * (errs[(size_t)h * P + y * W + x] - a->inlier_thresh);
                st = 1 / (1 + exp(-st));
                double dRE = -st * (1 - st) * a->inlier_beta * sgrad[h];
                dRE *= scale;
                int px, py;
                px_of(a, x, y, &px, &py);
                double dPdO[3];
                dproject_dobj((float)px, (float)py, sc_at(a, expert, 0, y, x), sc_at(a, expert, 1, y, x),
                              sc_at(a, expert, 2, y, x), R, pose + 3, a, a->max_reproj, dPdO);
                for (int cc = 0; cc < 3; cc++) g2[(size_t)(y * W + x) * 3 + cc] = dPdO[cc] * dRE;
                const double* dPdH = JH + ((size_t)h * P + (size_t)x * H + y) * 6;
                double tmp[6];
                for (int k = 0; k < 6; k++) tmp[k] = dRE * dPdH[k];
                for (int m = 0; m < 12; m++) {
                    double s = 0;
                    for (int k = 0; k < 6; k++) s += tmp[k] * dHdO[k * 12 + m];
                    support[m] += s;
                }
                if (b->out_support_raw)
                    for (int m = 0; m < 12; m++) {
                        double s = 0;
                        for (int k = 0; k < 6; k++) s += tmp[k] * dHdO_raw[k * 12 + m];
                        support_raw[m] += s;
                    }
            }
        if (b->out_grad_direct) memcpy(b->out_grad_direct + (size_t)h * P * 3, g2, (size_t)P * 3 * sizeof(double));
        if (b->out_support) memcpy(b->out_support + 12 * (size_t)h, support, sizeof(support));
        if (b->out_support_raw) memcpy(b->out_support_raw + 12 * (size_t)h, support_raw, sizeof(support_raw));
        for (int j = 0; j < 4; j++) {
            const int x = sxy[8 * h + 2 * j], y = sxy[8 * h + 2 * j + 1];
            for (int cc = 0; cc < 3; cc++) g2[(size_t)(y * W + x) * 3 + cc] += support[3 * j + cc];
        }
    }

    /* ---- assemble (esac.cpp:491-508): float += double, hypotheses in order ---- */
    for (int h = 0; h < N; h++) {
        if (probs[h] < PROB_THRESH_REF) continue;
        const int expert = (int)assign_at(a, h);
        for (int idx = 0; idx < P; idx++) {
            const int x = idx % W, y = idx / W;
            for (int cc = 0; cc < 3; cc++) {
                float* o = b->out_gradients + expert * b->grad_stride[0] + cc * b->grad_stride[1] + y * b->grad_stride[2] + x * b->grad_stride[3];
                *o += probs[h] * gradI[((size_t)h * P + idx) * 3 + cc] + gradII[((size_t)h * P + idx) * 3 + cc];
            }
        }
    }


    if (b->out_dloss) memcpy(b->out_dloss, dl_all, (size_t)N * 6 * sizeof(double));
    if (b->out_grad_path1) memcpy(b->out_grad_path1, gradI, (size_t)N * P * 3 * sizeof(double));
    if (b->out_grad_path2) memcpy(b->out_grad_path2, gradII, (size_t)N * P * 3 * sizeof(double));
    free(errs_own); free(JH_own); free(gradI); free(gradII); free(sgrad); free(dl_all);
}

static int bwd_threads(const esac_oracle_args* a) {
#ifdef _OPENMP
    int nthreads = a->num_threads > 0 ? a->num_threads : omp_get_max_threads();
    if (a->rng_mode == ESAC_RNG_CALLBACK) nthreads = 1;
    return nthreads;
#else
    (void)a;
    return 1;
#endif
}

int esac_oracle_backward_paths(esac_oracle_bwd_args* b, const esac_oracle_bwd_stages* st) {
    esac_oracle_args* a = &b->fwd;
    if (!a->scene_coords || !a->hyp_assign || a->N <= 0 || a->H < 3 || a->W < 3 || a->E <= 0 || !b->gt_pose || !b->out_gradients)
        return -1;
    if (!st || !st->init_hyps || !st->ref_hyps || !st->sample_xy || !st->probs || !st->losses || !st->have_map || !st->maps) return -1;
    ctx_t c;
    c.a = a;
    c.fx = c.fy = (double)a->focal; c.cx = (double)a->ppx; c.cy = (double)a->ppy;
    backward_paths(&c, b, st, NULL, NULL, bwd_threads(a));
    return 0;
}

double esac_oracle_backward(esac_oracle_bwd_args* b) {
    esac_oracle_args* a = &b->fwd;
    if (!a->scene_coords || !a->hyp_assign || a->N <= 0 || a->H < 3 || a->W < 3 || a->E <= 0 || !b->gt_pose || !b->out_gradients)
        return -1.0;
    const int N = a->N, H = a->H, W = a->W, P = H * W;
    const int max_tries = a->max_tries > 0 ? a->max_tries : ESAC_ORACLE_MAX_TRIES;
    const int max_ref = a->max_ref_steps >= 0 ? a->max_ref_steps : ESAC_ORACLE_MAX_REF_STEPS;
    const int nthreads = bwd_threads(a);
    (void)nthreads;
    ctx_t c;
    c.a = a;
    c.fx = c.fy = (double)a->focal; c.cx = (double)a->ppx; c.cy = (double)a->ppy;
    const double wRot = (double)b->w_rot, wTrans = (double)b->w_trans, cut = (double)b->loss_cut;
    double gtT[16];
    for (int i = 0; i < 16; i++) gtT[i] = (double)b->gt_pose[i];

    double* initHyps = (double*)calloc((size_t)N * 6, sizeof(double));
    double* refHyps = (double*)calloc((size_t)N * 6, sizeof(double));
    int32_t* sxy = (int32_t*)calloc((size_t)N * 8, sizeof(int32_t));
    float* errs = (float*)malloc((size_t)N * P * sizeof(float));
    double* JH = (double*)malloc((size_t)N * P * 6 * sizeof(double));
    uint8_t* maps = (uint8_t*)calloc((size_t)N * P, 1);
    uint8_t* have_map = (uint8_t*)calloc((size_t)N, 1);
    double* scores = (double*)calloc((size_t)N, sizeof(double));
    double* probs = (double*)calloc((size_t)N, sizeof(double));
    double* losses = (double*)calloc((size_t)N, sizeof(double));
    int32_t* ref_steps = (int32_t*)calloc((size_t)N, sizeof(int32_t));
    int32_t* ref_inliers = (int32_t*)calloc((size_t)N, sizeof(int32_t));
    int32_t* ref_lm = (int32_t*)calloc((size_t)N, sizeof(int32_t));

    /* ---- sampleHypotheses (esac.cpp:276) ---- */
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
    for (int h = 0; h < N; h++) {
        int expert = (int)assign_at(a, h);
        for (int t = 0; t < max_tries; t++)
            if (sample_try(&c, h, expert, (uint32_t)t, sxy + 8 * h, initHyps + 6 * h)) break;
    }
    /* ---- reprojection errors + Jacobians, scores, softmax (esac.cpp:295-319) ---- */
#pragma omp parallel for schedule(static) num_threads(nthreads)
    for (int h = 0; h < N; h++)
        repro_errs_jac(&c, initHyps + 6 * h, (int)assign_at(a, h), errs + (size_t)h * P, JH + (size_t)h * P * 6);
#pragma omp parallel for schedule(static) num_threads(nthreads)
    for (int h = 0; h < N; h++) scores[h] = hyp_score_from_errs(a, errs + (size_t)h * P);
    soft_max(scores, N, probs);
    const double ent = entropy(probs, N);

    /* ---- refine every hypothesis with prob >= PROB_THRESH (esac.cpp:328-347) ---- */
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
    for (int h = 0; h < N; h++) {
        memcpy(refHyps + 6 * h, initHyps + 6 * h, 6 * sizeof(double));
        if (probs[h] < PROB_THRESH_REF) continue;
        int32_t* counts = (int32_t*)calloc((size_t)max_ref + 1, sizeof(int32_t));
        int acc = refine_hyp(&c, errs + (size_t)h * P, (int)assign_at(a, h), max_ref, refHyps + 6 * h, maps + (size_t)h * P, counts, ref_lm + h);
        have_map[h] = acc > 0; /* inlierMaps[h] stays an empty Mat when no re-fit was accepted */
        ref_steps[h] = acc;
        ref_inliers[h] = acc > 0 ? counts[acc - 1] : 0; /* the inlier set the last accepted re-fit ran on */
        free(counts);
    }
    /* ---- expected loss (esac.cpp:354-362) ---- */
    double expectedLoss = 0;
    for (int h = 0; h < N; h++) {
        double T[16];
        esac_oracle_pose2trans(refHyps + 6 * h, T);
        losses[h] = loss_fn(T, gtT, wRot, wTrans, cut);
        expectedLoss += probs[h] * losses[h];
    }

    /* ---- path I, path II, assemble (esac.cpp:375-508): a function of the stages above ---- */
    esac_oracle_bwd_stages st;
    memset(&st, 0, sizeof(st));
    st.init_hyps = initHyps; st.ref_hyps = refHyps; st.sample_xy = sxy; st.probs = probs; st.losses = losses;
    st.have_map = have_map; st.maps = maps;
    backward_paths(&c, b, &st, errs, JH, nthreads);

    if (b->out_probs) memcpy(b->out_probs, probs, (size_t)N * sizeof(double));
    if (b->out_losses) memcpy(b->out_losses, losses, (size_t)N * sizeof(double));
    if (b->out_init_hyps) memcpy(b->out_init_hyps, initHyps, (size_t)N * 6 * sizeof(double));
    if (b->out_ref_hyps) memcpy(b->out_ref_hyps, refHyps, (size_t)N * 6 * sizeof(double));
    if (b->out_sample_xy) memcpy(b->out_sample_xy, sxy, (size_t)N * 8 * sizeof(int32_t));
    if (b->out_entropy) *b->out_entropy = ent;
    if (b->out_scores) memcpy(b->out_scores, scores, (size_t)N * sizeof(double));
    if (b->out_maps) memcpy(b->out_maps, maps, (size_t)N * P);
    if (b->out_have_map) memcpy(b->out_have_map, have_map, (size_t)N);
    if (b->out_ref_steps) memcpy(b->out_ref_steps, ref_steps, (size_t)N * sizeof(int32_t));
    if (b->out_ref_inliers) memcpy(b->out_ref_inliers, ref_inliers, (size_t)N * sizeof(int32_t));
    if (b->out_ref_lm_iters) memcpy(b->out_ref_lm_iters, ref_lm, (size_t)N * sizeof(int32_t));

    free(initHyps); free(refHyps); free(sxy); free(errs); free(JH); free(maps); free(have_map); free(scores);
    free(probs); free(losses); free(ref_steps); free(ref_inliers); free(ref_lm);
    return expectedLoss;
}

/* ---- small-routine exports (tests compare the HIP library's host-compiled math against these) ---- */
double esac_oracle_pose_loss(const double pose[6], const double gt_trans[16], double wRot, double wTrans, double cut) {
    double T[16];
    esac_oracle_pose2trans(pose, T);
    return loss_fn(T, gt_trans, wRot, wTrans, cut);
}
void esac_oracle_pose_dloss(const double est[6], const double gt_pose[6], double wRot, double wTrans, double cut, double jac[6]) {
    dloss_fn(est, gt_pose, wRot, wTrans, cut, jac);
}
void esac_oracle_trans2pose(const double T[16], double pose[6]) { trans2pose_fn(T, pose); }
void esac_oracle_soft_max(const double* scores, int n, double* probs) { soft_max(scores, n, probs); }
void esac_oracle_dproject_dobj(float ptx, float pty, float ox, float oy, float oz, const double rvec[3], const double t[3],
                               float focal, float ppx, float ppy, float maxReproj, double out[3]) {
    esac_oracle_args a;
    memset(&a, 0, sizeof(a));
    a.focal = focal; a.ppx = ppx; a.ppy = ppy;
    double R[9];
    esac_oracle_rodrigues_vec2mat(rvec, R, NULL);
    dproject_dobj(ptx, pty, ox, oy, oz, R, t, &a, maxReproj, out);
}
int esac_oracle_norm_jac_row(const double rvec[3], const double t[3], float focal, float ppx, float ppy, float X, float Y,
                             float Z, float px, float py, float maxReproj, double row[6]) {
    esac_oracle_args a;
    memset(&a, 0, sizeof(a));
    ctx_t c;
    c.a = &a;
    c.fx = c.fy = (double)focal; c.cx = (double)ppx; c.cy = (double)ppy;
    double R[9], dRdr[27];
    esac_oracle_rodrigues_vec2mat(rvec, R, dRdr);
    return norm_jac_row(R, dRdr, t, &c, X, Y, Z, px, py, maxReproj, row);
}
