/* front_end_odom_ref.c - the checker of odomDeskewInfo(), positional deskew and the initial pose guess: a plain C
 * restatement of the reference's src/imageProjection.cpp odomDeskewInfo() :411-491, findPosition() :520-534 WITH its
 * commented lines live, deskewPoint() :536-566 and projectPointCloud() :568-598 with that position, and of
 * src/mapOptmization.cpp updateInitialGuess() :899-958. Test infrastructure: compiled with `gcc -O2 -ffp-contract=off` by
 * tests/ref/front_end_odom_ref.py, loaded with ctypes; it calls the host's libm. Nothing here is shared with the product.
 * Assumptions about code outside the reference (tf, PCL, Eigen) are written where they are used. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* ---- small float transforms, row-major 4x4 ---------------------------------------------------------------------------- */
/* pcl::getTransformation(x, y, z, roll, pitch, yaw) (PCL 1.10 common/impl/eigen.hpp): float parameters */
static void get_transformation(float x, float y, float z, float roll, float pitch, float yaw, float t[16])
{
    float A = cosf(yaw), B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll), F = sinf(roll), DE = D * E, DF = D * F;
    t[0] = A * C;  t[1] = A * DF - B * E;  t[2] = B * F + A * DE;   t[3] = x;
    t[4] = B * C;  t[5] = A * E + B * DF;  t[6] = B * DE - A * F;   t[7] = y;
    t[8] = -D;     t[9] = C * F;           t[10] = C * E;           t[11] = z;
    t[12] = 0;     t[13] = 0;              t[14] = 0;               t[15] = 1;
}

/* Eigen 3.3 Transform<float,3,Affine>::inverse(): compute_inverse<Matrix3f> (cofactors, 1/det from column 0), translation
 * -(Linv * t) */
static float cofactor(const float m[16], int i, int j)
{
    int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 4 + j1] * m[i2 * 4 + j2] - m[i1 * 4 + j2] * m[i2 * 4 + j1];
}
static void affine_inverse(const float m[16], float r[16])
{
    float c0 = cofactor(m, 0, 0), c1 = cofactor(m, 1, 0), c2 = cofactor(m, 2, 0);
    float det = (c0 * m[0] + c1 * m[4]) + c2 * m[8];
    float invdet = 1.0f / det;
    r[0] = c0 * invdet;
    r[1] = c1 * invdet;
    r[2] = c2 * invdet;
    for (int c = 0; c < 3; c++) {
        r[4 + c] = cofactor(m, c, 1) * invdet;
        r[8 + c] = cofactor(m, c, 2) * invdet;
    }
    for (int i = 0; i < 3; i++) r[i * 4 + 3] = -((r[i * 4 + 0] * m[3] + r[i * 4 + 1] * m[7]) + r[i * 4 + 2] * m[11]);
    r[12] = 0; r[13] = 0; r[14] = 0; r[15] = 1;
}
/* the Affine3f product as a 4x4 product, ((a0 b0 + a1 b1) + a2 b2) + a3 b3: imageProjection's convention here */
static void mul4x4(const float a[16], const float b[16], float r[16])
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            r[i * 4 + j] = ((a[i * 4 + 0] * b[0 * 4 + j] + a[i * 4 + 1] * b[1 * 4 + j]) + a[i * 4 + 2] * b[2 * 4 + j]) + a[i * 4 + 3] * b[3 * 4 + j];
}
/* the Affine3f product as Eigen's affine form, linear = L * L (three terms), translation = L * t + t: mapOptimization's
 * convention here */
static void mul_affine(const float a[16], const float b[16], float r[16])
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) r[i * 4 + j] = (a[i * 4 + 0] * b[0 * 4 + j] + a[i * 4 + 1] * b[1 * 4 + j]) + a[i * 4 + 2] * b[2 * 4 + j];
        r[i * 4 + 3] = ((a[i * 4 + 0] * b[3] + a[i * 4 + 1] * b[7]) + a[i * 4 + 2] * b[11]) + a[i * 4 + 3];
    }
    r[12] = 0; r[13] = 0; r[14] = 0; r[15] = 1;
}
/* pcl::getTranslationAndEulerAngles (PCL 1.10) in float */
static void get_translation_and_euler(const float t[16], float *x, float *y, float *z, float *roll, float *pitch, float *yaw)
{
    *x = t[3];
    *y = t[7];
    *z = t[11];
    *roll = atan2f(t[9], t[10]);
    *pitch = asinf(-t[8]);
    *yaw = atan2f(t[4], t[0]);
}

/* tf::Matrix3x3(q).getRPY(roll, pitch, yaw) in double: setRotation (s = 2 / length2), getEulerYPR solution 1 */
static void quaternion_rpy(double x, double y, double z, double w, double *roll, double *pitch, double *yaw)
{
    double d = x * x + y * y + z * z + w * w;
    double s = 2.0 / d;
    double xs = x * s, ys = y * s, zs = z * s;
    double wx = w * xs, wy = w * ys, wz = w * zs;
    double xx = x * xs, xy = x * ys, xz = x * zs;
    double yy = y * ys, yz = y * zs, zz = z * zs;
    double m[3][3] = { { 1.0 - (yy + zz), xy - wz, xz + wy }, { xy + wz, 1.0 - (xx + zz), yz - wx }, { xz - wy, yz + wx, 1.0 - (xx + yy) } };
    if (fabs(m[2][0]) >= 1) {
        *yaw = 0;
        if (m[2][0] < 0) {
            *pitch = M_PI / 2.0;
            *roll = atan2(m[0][1], m[0][2]);
        } else {
            *pitch = -M_PI / 2.0;
            *roll = atan2(-m[0][1], -m[0][2]);
        }
    } else {
        *pitch = -asin(m[2][0]);
        *roll = atan2(m[2][1] / cos(*pitch), m[2][2] / cos(*pitch));
        *yaw = atan2(m[1][0] / cos(*pitch), m[0][0] / cos(*pitch));
    }
}

/* ---- odomDeskewInfo() :411-491 ------------------------------------------------------------------------------------------ */
typedef struct { double time, px, py, pz, qx, qy, qz, qw, cov0; } ref_odom;
typedef struct {
    int32_t odomAvailable, odomDeskewFlag;
    float initialGuess[6]; /* X Y Z Roll Pitch Yaw */
    float odomIncre[3];
    int32_t popped;
} ref_odom_out;

void ref_odom_deskew_info(const ref_odom *queue, size_t size, double timeScanCur, double timeScanEnd, float imuRate, ref_odom_out *o)
{
    memset(o, 0, sizeof(*o)); /* :413; members of a fresh node */
    float sync_diff_time = (imuRate >= 300) ? 0.01 : 0.20; /* :414 */
    size_t head = 0;
    while (head < size) { /* :415-421 */
        if (queue[head].time < timeScanCur - sync_diff_time) head++;
        else break;
    }
    o->popped = (int32_t)head;
    if (head == size) return; /* :423-424 */
    if (queue[head].time > timeScanCur) return; /* :426-427 */
    ref_odom startOdomMsg = queue[head];
    for (int i = (int)head; i < (int)size; ++i) { /* :432-440 */
        startOdomMsg = queue[i];
        if (startOdomMsg.time < timeScanCur) continue;
        else break;
    }
    double roll, pitch, yaw;
    quaternion_rpy(startOdomMsg.qx, startOdomMsg.qy, startOdomMsg.qz, startOdomMsg.qw, &roll, &pitch, &yaw); /* :442-446 */
    o->initialGuess[0] = startOdomMsg.px; /* :449-454 */
    o->initialGuess[1] = startOdomMsg.py;
    o->initialGuess[2] = startOdomMsg.pz;
    o->initialGuess[3] = roll;
    o->initialGuess[4] = pitch;
    o->initialGuess[5] = yaw;
    o->odomAvailable = 1; /* :456 */
    o->odomDeskewFlag = 0; /* :459 */
    if (queue[size - 1].time < timeScanEnd) return; /* :461-462 */
    ref_odom endOdomMsg = queue[head];
    for (int i = (int)head; i < (int)size; ++i) { /* :466-474 */
        endOdomMsg = queue[i];
        if (endOdomMsg.time < timeScanEnd) continue;
        else break;
    }
    if ((int)round(startOdomMsg.cov0) != (int)round(endOdomMsg.cov0)) return; /* :476-477 */
    float transBegin[16], transEnd[16], inv[16], transBt[16];
    get_transformation(startOdomMsg.px, startOdomMsg.py, startOdomMsg.pz, roll, pitch, yaw, transBegin); /* :479 */
    quaternion_rpy(endOdomMsg.qx, endOdomMsg.qy, endOdomMsg.qz, endOdomMsg.qw, &roll, &pitch, &yaw); /* :481-482 */
    get_transformation(endOdomMsg.px, endOdomMsg.py, endOdomMsg.pz, roll, pitch, yaw, transEnd); /* :483 */
    affine_inverse(transBegin, inv);
    mul4x4(inv, transEnd, transBt); /* :485 */
    float rollIncre, pitchIncre, yawIncre;
    get_translation_and_euler(transBt, &o->odomIncre[0], &o->odomIncre[1], &o->odomIncre[2], &rollIncre, &pitchIncre, &yawIncre); /* :488 */
    o->odomDeskewFlag = 1; /* :490 */
}

/* ---- projectPointCloud() with findPosition() live ----------------------------------------------------------------------- */
typedef struct {
    uint32_t stride, off_x, off_intensity, off_ring, off_time;
    int32_t ring_type; /* 0 u8, 1 u16, 2 i32 */
    int32_t time_type; /* 0 f32, 1 u32 ns, 2 u32, 3 f64 relative to record 0 */
} ref_layout;

typedef struct {
    double timeScanCur, timeScanEnd;
    int deskew; /* deskewFlag == 1 && cloudInfo.imuAvailable */
    int imuPointerCur;
    const double *imuTime, *imuRotX, *imuRotY, *imuRotZ;
    int position; /* cloudInfo.odomAvailable && odomDeskewFlag (:526) */
    float odomIncreX, odomIncreY, odomIncreZ;
    int firstPointFlag;
    float transStartInverse[16];
} ref_node;

static void findRotation(const ref_node *s, double pointTime, float *rotXCur, float *rotYCur, float *rotZCur) /* :493-518 */
{
    *rotXCur = 0; *rotYCur = 0; *rotZCur = 0;
    int imuPointerFront = 0;
    while (imuPointerFront < s->imuPointerCur) {
        if (pointTime < s->imuTime[imuPointerFront]) break;
        ++imuPointerFront;
    }
    if (pointTime > s->imuTime[imuPointerFront] || imuPointerFront == 0) {
        *rotXCur = s->imuRotX[imuPointerFront];
        *rotYCur = s->imuRotY[imuPointerFront];
        *rotZCur = s->imuRotZ[imuPointerFront];
    } else {
        int imuPointerBack = imuPointerFront - 1;
        double ratioFront = (pointTime - s->imuTime[imuPointerBack]) / (s->imuTime[imuPointerFront] - s->imuTime[imuPointerBack]);
        double ratioBack = (s->imuTime[imuPointerFront] - pointTime) / (s->imuTime[imuPointerFront] - s->imuTime[imuPointerBack]);
        *rotXCur = s->imuRotX[imuPointerFront] * ratioFront + s->imuRotX[imuPointerBack] * ratioBack;
        *rotYCur = s->imuRotY[imuPointerFront] * ratioFront + s->imuRotY[imuPointerBack] * ratioBack;
        *rotZCur = s->imuRotZ[imuPointerFront] * ratioFront + s->imuRotZ[imuPointerBack] * ratioBack;
    }
}

static void findPosition(const ref_node *s, double relTime, float *posXCur, float *posYCur, float *posZCur) /* :520-534, the comments live */
{
    *posXCur = 0; *posYCur = 0; *posZCur = 0;
    if (!s->position) return; /* :526-527 */
    float ratio = relTime / (s->timeScanEnd - s->timeScanCur); /* :529 */
    *posXCur = ratio * s->odomIncreX; /* :531-533 */
    *posYCur = ratio * s->odomIncreY;
    *posZCur = ratio * s->odomIncreZ;
}

static void deskewPoint(ref_node *s, const float in[4], double relTime, float out[4]) /* :536-566 */
{
    if (!s->deskew) {
        memcpy(out, in, 16);
        return;
    }
    double pointTime = s->timeScanCur + relTime;
    float rotXCur, rotYCur, rotZCur;
    findRotation(s, pointTime, &rotXCur, &rotYCur, &rotZCur);
    float posXCur, posYCur, posZCur;
    findPosition(s, relTime, &posXCur, &posYCur, &posZCur);
    if (s->firstPointFlag) {
        float first[16];
        get_transformation(posXCur, posYCur, posZCur, rotXCur, rotYCur, rotZCur, first);
        affine_inverse(first, s->transStartInverse);
        s->firstPointFlag = 0;
    }
    float transFinal[16], transBt[16];
    get_transformation(posXCur, posYCur, posZCur, rotXCur, rotYCur, rotZCur, transFinal);
    mul4x4(s->transStartInverse, transFinal, transBt);
    out[0] = transBt[0] * in[0] + transBt[1] * in[1] + transBt[2] * in[2] + transBt[3];
    out[1] = transBt[4] * in[0] + transBt[5] * in[1] + transBt[6] * in[2] + transBt[7];
    out[2] = transBt[8] * in[0] + transBt[9] * in[1] + transBt[10] * in[2] + transBt[11];
    out[3] = in[3];
}

/* The conversion loops (:216-274) and projectPointCloud() (:568-598) over the raw records. out: 8 floats per survivor
 * {x, y, z, 0, intensity, 0, 0, 0}; returns fullCloud->size(). */
size_t ref_project_motion(const unsigned char *pts, size_t n, const ref_layout *l, int N_SCAN, int downsampleRate, int point_filter_num,
                          float lidarMinRange, float lidarMaxRange, int deskew, double timeScanCur, int imuPointerCur, const double *imuTime,
                          const double *imuRotX, const double *imuRotY, const double *imuRotZ, int position, double timeScanEnd,
                          const float *odomIncre, float *out)
{
    ref_node s;
    memset(&s, 0, sizeof(s));
    s.timeScanCur = timeScanCur; s.timeScanEnd = timeScanEnd;
    s.deskew = deskew;
    s.imuPointerCur = imuPointerCur;
    s.imuTime = imuTime; s.imuRotX = imuRotX; s.imuRotY = imuRotY; s.imuRotZ = imuRotZ;
    s.position = position;
    s.odomIncreX = odomIncre[0]; s.odomIncreY = odomIncre[1]; s.odomIncreZ = odomIncre[2];
    s.firstPointFlag = 1;
    double start_stamptime = 0;
    if (n > 0 && l->time_type == 3) memcpy(&start_stamptime, pts + l->off_time, 8);
    size_t m = 0;
    int cloudSize = (int)n;
    for (int i = 0; i < cloudSize; ++i) {
        const unsigned char *src = pts + (size_t)i * l->stride;
        float p[4], time;
        memcpy(p, src + l->off_x, 12);
        memcpy(&p[3], src + l->off_intensity, 4);
        int ring;
        if (l->ring_type == 0) ring = src[l->off_ring];
        else if (l->ring_type == 1) { uint16_t r; memcpy(&r, src + l->off_ring, 2); ring = r; }
        else { int32_t r; memcpy(&r, src + l->off_ring, 4); ring = r; }
        if (l->time_type == 0) memcpy(&time, src + l->off_time, 4);
        else if (l->time_type == 1) { uint32_t t; memcpy(&t, src + l->off_time, 4); time = t * 1e-9f; }
        else if (l->time_type == 2) { uint32_t t; memcpy(&t, src + l->off_time, 4); time = (float)t; }
        else { double t; memcpy(&t, src + l->off_time, 8); time = t - start_stamptime; }
        float range = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        if (range < lidarMinRange || range > lidarMaxRange) continue;
        int rowIdn = ring;
        if (rowIdn < 0 || rowIdn >= N_SCAN) continue;
        if (rowIdn % downsampleRate != 0) continue;
        if (i % point_filter_num != 0) continue;
        float q[4];
        deskewPoint(&s, p, time, q);
        float *o = out + 8 * m++;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = 0; o[4] = q[3]; o[5] = 0; o[6] = 0; o[7] = 0;
    }
    return m;
}

/* ---- updateInitialGuess() src/mapOptmization.cpp:899-958 ---------------------------------------------------------------- */
typedef struct {
    float lastImuTransformation[16];
    float lastImuPreTransformation[16];
    int lastImuPreTransAvailable;
} ref_guess_state;
typedef struct {
    int64_t imuAvailable, odomAvailable;
    float imuRollInit, imuPitchInit, imuYawInit;
    float initialGuessX, initialGuessY, initialGuessZ, initialGuessRoll, initialGuessPitch, initialGuessYaw;
} ref_cloud_info;

void ref_guess_state_init(ref_guess_state *st) { memset(st, 0, sizeof(*st)); } /* function statics: zero storage, flag false */

static void trans2Affine3f(const float t[6], float out[16]) { get_transformation(t[3], t[4], t[5], t[0], t[1], t[2], out); } /* :348-351 */

void ref_update_initial_guess(ref_guess_state *st, float transformTobeMapped[6], int keyPosesEmpty, const ref_cloud_info *cloudInfo,
                              int useImuHeadingInitialization, int imuType, float incrementalOdometryAffineFront[16])
{
    trans2Affine3f(transformTobeMapped, incrementalOdometryAffineFront); /* :902 */
    if (keyPosesEmpty) { /* :906-917 */
        transformTobeMapped[0] = cloudInfo->imuRollInit;
        transformTobeMapped[1] = cloudInfo->imuPitchInit;
        transformTobeMapped[2] = cloudInfo->imuYawInit;
        if (!useImuHeadingInitialization) transformTobeMapped[2] = 0;
        get_transformation(0, 0, 0, cloudInfo->imuRollInit, cloudInfo->imuPitchInit, cloudInfo->imuYawInit, st->lastImuTransformation);
        return;
    }
    if (cloudInfo->odomAvailable == 1) { /* :922 */
        float transBack[16];
        get_transformation(cloudInfo->initialGuessX, cloudInfo->initialGuessY, cloudInfo->initialGuessZ, cloudInfo->initialGuessRoll,
                           cloudInfo->initialGuessPitch, cloudInfo->initialGuessYaw, transBack);
        if (st->lastImuPreTransAvailable == 0) { /* :926-929 */
            memcpy(st->lastImuPreTransformation, transBack, sizeof(transBack));
            st->lastImuPreTransAvailable = 1;
        } else { /* :930-941 */
            float inv[16], transIncre[16], transTobe[16], transFinal[16];
            affine_inverse(st->lastImuPreTransformation, inv);
            mul_affine(inv, transBack, transIncre);
            trans2Affine3f(transformTobeMapped, transTobe);
            mul_affine(transTobe, transIncre, transFinal);
            get_translation_and_euler(transFinal, &transformTobeMapped[3], &transformTobeMapped[4], &transformTobeMapped[5],
                                      &transformTobeMapped[0], &transformTobeMapped[1], &transformTobeMapped[2]);
            memcpy(st->lastImuPreTransformation, transBack, sizeof(transBack));
            get_transformation(0, 0, 0, cloudInfo->imuRollInit, cloudInfo->imuPitchInit, cloudInfo->imuYawInit, st->lastImuTransformation);
            return;
        }
    }
    if (cloudInfo->imuAvailable == 1 && imuType) { /* :945-957 */
        float transBack[16], inv[16], transIncre[16], transTobe[16], transFinal[16];
        get_transformation(0, 0, 0, cloudInfo->imuRollInit, cloudInfo->imuPitchInit, cloudInfo->imuYawInit, transBack);
        affine_inverse(st->lastImuTransformation, inv);
        mul_affine(inv, transBack, transIncre);
        trans2Affine3f(transformTobeMapped, transTobe);
        mul_affine(transTobe, transIncre, transFinal);
        get_translation_and_euler(transFinal, &transformTobeMapped[3], &transformTobeMapped[4], &transformTobeMapped[5],
                                  &transformTobeMapped[0], &transformTobeMapped[1], &transformTobeMapped[2]);
        get_transformation(0, 0, 0, cloudInfo->imuRollInit, cloudInfo->imuPitchInit, cloudInfo->imuYawInit, st->lastImuTransformation);
        return;
    }
}
