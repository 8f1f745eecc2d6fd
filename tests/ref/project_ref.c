/* project_ref.c - the checker of the point filter and IMU deskew: a plain C restatement of the reference's
 * src/imageProjection.cpp, conversion loops :216-274, imuDeskewInfo() :350-409, findRotation() :493-518, deskewPoint()
 * :536-566, projectPointCloud() :568-598. Test infrastructure: compiled with `gcc -O2 -ffp-contract=off` by
 * tests/ref/build_ref.py, loaded with ctypes; it calls the host's sinf / cosf. Nothing here is shared with the product. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define QUEUE_LENGTH 2000 /* :62 */

typedef struct {
    uint32_t stride, off_x, off_intensity, off_ring, off_time;
    int32_t ring_type; /* 0 u8, 1 u16, 2 i32 */
    int32_t time_type; /* 0 f32, 1 u32 ns, 2 u32, 3 f64 relative to record 0 */
} ref_layout;

typedef struct {
    double time_scan_cur;
    int deskew; /* deskewFlag == 1 && cloudInfo.imuAvailable */
    int imu_pointer_cur;
    const double *imu_time, *imu_rot_x, *imu_rot_y, *imu_rot_z;
    int first_point_flag;
    float start_inverse[16]; /* transStartInverse, row-major 4x4 */
} ref_state;

/* imuDeskewInfo() :350-409 (the queue already popped, no imuType lines). Returns -5 where the reference would write
 * past its arrays of queueLength entries. */
int ref_imu_deskew_info(const double *imu, size_t n, double time_scan_cur, double time_scan_end, double *imu_time, double *rot_x,
                        double *rot_y, double *rot_z, int32_t *pointer_cur, int32_t *available)
{
    (void)time_scan_cur;
    *available = 0; /* :352 */
    *pointer_cur = 0;
    if (n == 0) return 0; /* :362-363 */
    int imuPointerCur = 0; /* :365 */
    for (int i = 0; i < (int)n; ++i) { /* :367 */
        double currentImuTime = imu[4 * i]; /* :370 */
        if (currentImuTime > time_scan_end + 0.01) break; /* :378-379 */
        if (imuPointerCur >= QUEUE_LENGTH) return -5;
        if (imuPointerCur == 0) { /* :381-388 */
            rot_x[0] = 0;
            rot_y[0] = 0;
            rot_z[0] = 0;
            imu_time[0] = currentImuTime;
            ++imuPointerCur;
            continue;
        }
        double angular_x = imu[4 * i + 1], angular_y = imu[4 * i + 2], angular_z = imu[4 * i + 3]; /* :391-392 */
        double timeDiff = currentImuTime - imu_time[imuPointerCur - 1]; /* :395 */
        rot_x[imuPointerCur] = rot_x[imuPointerCur - 1] + angular_x * timeDiff; /* :396-398 */
        rot_y[imuPointerCur] = rot_y[imuPointerCur - 1] + angular_y * timeDiff;
        rot_z[imuPointerCur] = rot_z[imuPointerCur - 1] + angular_z * timeDiff;
        imu_time[imuPointerCur] = currentImuTime; /* :399 */
        ++imuPointerCur; /* :400 */
    }
    --imuPointerCur; /* :403 */
    *pointer_cur = imuPointerCur;
    if (imuPointerCur <= 0) return 0; /* :405-406 */
    *available = 1; /* :408 */
    return 0;
}

/* findRotation() :493-518, the linear walk as written */
static void find_rotation(const ref_state *s, double pointTime, float *rotXCur, float *rotYCur, float *rotZCur)
{
    *rotXCur = 0;
    *rotYCur = 0;
    *rotZCur = 0;
    int imuPointerFront = 0;
    while (imuPointerFront < s->imu_pointer_cur) {
        if (pointTime < s->imu_time[imuPointerFront]) break;
        ++imuPointerFront;
    }
    if (pointTime > s->imu_time[imuPointerFront] || imuPointerFront == 0) {
        *rotXCur = s->imu_rot_x[imuPointerFront];
        *rotYCur = s->imu_rot_y[imuPointerFront];
        *rotZCur = s->imu_rot_z[imuPointerFront];
    } else {
        int imuPointerBack = imuPointerFront - 1;
        double ratioFront = (pointTime - s->imu_time[imuPointerBack]) / (s->imu_time[imuPointerFront] - s->imu_time[imuPointerBack]);
        double ratioBack = (s->imu_time[imuPointerFront] - pointTime) / (s->imu_time[imuPointerFront] - s->imu_time[imuPointerBack]);
        *rotXCur = s->imu_rot_x[imuPointerFront] * ratioFront + s->imu_rot_x[imuPointerBack] * ratioBack;
        *rotYCur = s->imu_rot_y[imuPointerFront] * ratioFront + s->imu_rot_y[imuPointerBack] * ratioBack;
        *rotZCur = s->imu_rot_z[imuPointerFront] * ratioFront + s->imu_rot_z[imuPointerBack] * ratioBack;
    }
}

/* pcl::getTransformation(x, y, z, roll, pitch, yaw) (PCL 1.10 common/impl/eigen.hpp), float, row-major 4x4 */
static void get_transformation(float x, float y, float z, float roll, float pitch, float yaw, float t[16])
{
    float A = cosf(yaw), B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll), F = sinf(roll), DE = D * E, DF = D * F;
    t[0] = A * C;  t[1] = A * DF - B * E;  t[2] = B * F + A * DE;   t[3] = x;
    t[4] = B * C;  t[5] = A * E + B * DF;  t[6] = B * DE - A * F;   t[7] = y;
    t[8] = -D;     t[9] = C * F;           t[10] = C * E;           t[11] = z;
    t[12] = 0;     t[13] = 0;              t[14] = 0;               t[15] = 1;
}

/* Eigen 3.3 Transform<float,3,Affine>::inverse(): linear part by compute_inverse<Matrix3f> (cofactors, 1/det from column
 * 0), translation -(Linv * t), last row (0, 0, 0, 1) */
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
    r[12] = 0;
    r[13] = 0;
    r[14] = 0;
    r[15] = 1;
}

/* deskewPoint() :536-566 */
static void deskew_point(ref_state *s, const float in[4], double relTime, float out[4])
{
    if (!s->deskew) { /* :538-539 */
        memcpy(out, in, 16);
        return;
    }
    double pointTime = s->time_scan_cur + relTime; /* :541 */
    float rotXCur, rotYCur, rotZCur;
    find_rotation(s, pointTime, &rotXCur, &rotYCur, &rotZCur); /* :544 */
    float posXCur = 0, posYCur = 0, posZCur = 0; /* findPosition() :520-534 */
    float transFinal[16], transBt[16];
    get_transformation(posXCur, posYCur, posZCur, rotXCur, rotYCur, rotZCur, transFinal); /* :551, :556 */
    if (s->first_point_flag) { /* :549-553 */
        affine_inverse(transFinal, s->start_inverse);
        s->first_point_flag = 0;
    }
    for (int i = 0; i < 4; i++) /* :557 */
        for (int j = 0; j < 4; j++)
            transBt[i * 4 + j] = ((s->start_inverse[i * 4 + 0] * transFinal[0 * 4 + j] + s->start_inverse[i * 4 + 1] * transFinal[1 * 4 + j]) +
                                  s->start_inverse[i * 4 + 2] * transFinal[2 * 4 + j]) + s->start_inverse[i * 4 + 3] * transFinal[3 * 4 + j];
    out[0] = transBt[0] * in[0] + transBt[1] * in[1] + transBt[2] * in[2] + transBt[3]; /* :560-562 */
    out[1] = transBt[4] * in[0] + transBt[5] * in[1] + transBt[6] * in[2] + transBt[7];
    out[2] = transBt[8] * in[0] + transBt[9] * in[1] + transBt[10] * in[2] + transBt[11];
    out[3] = in[3]; /* :563 */
}

/* The conversion loops (:216-274) and projectPointCloud() (:568-598) in one pass over the raw records. out: 8 floats per
 * survivor {x, y, z, 0, intensity, 0, 0, 0}; returns the number of survivors (fullCloud->size()). */
size_t ref_project(const unsigned char *pts, size_t n, const ref_layout *l, int N_SCAN, int downsampleRate, int point_filter_num,
                   float lidarMinRange, float lidarMaxRange, int deskew, double time_scan_cur, int imu_pointer_cur, const double *imu_time,
                   const double *rot_x, const double *rot_y, const double *rot_z, float *out)
{
    ref_state s;
    memset(&s, 0, sizeof(s));
    s.time_scan_cur = time_scan_cur;
    s.deskew = deskew;
    s.imu_pointer_cur = imu_pointer_cur;
    s.imu_time = imu_time; s.imu_rot_x = rot_x; s.imu_rot_y = rot_y; s.imu_rot_z = rot_z;
    s.first_point_flag = 1; /* resetParameters() :195 */
    double start_stamptime = 0; /* :263 */
    if (n > 0 && l->time_type == 3) memcpy(&start_stamptime, pts + l->off_time, 8);
    size_t m = 0;
    int cloudSize = (int)n; /* :570 */
    for (int i = 0; i < cloudSize; ++i) {
        const unsigned char *src = pts + (size_t)i * l->stride;
        float p[4], time; /* thisPoint {x, y, z, intensity} :574-578 */
        memcpy(p, src + l->off_x, 12);
        memcpy(&p[3], src + l->off_intensity, 4);
        int ring;
        if (l->ring_type == 0) ring = src[l->off_ring];
        else if (l->ring_type == 1) { uint16_t r; memcpy(&r, src + l->off_ring, 2); ring = r; }
        else { int32_t r; memcpy(&r, src + l->off_ring, 4); ring = r; }
        if (l->time_type == 0) memcpy(&time, src + l->off_time, 4); /* :216-219 */
        else if (l->time_type == 1) { uint32_t t; memcpy(&t, src + l->off_time, 4); time = t * 1e-9f; } /* :235 */
        else if (l->time_type == 2) { uint32_t t; memcpy(&t, src + l->off_time, 4); time = (float)t; } /* :253 */
        else { double t; memcpy(&t, src + l->off_time, 8); time = t - start_stamptime; } /* :272 */

        float range = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]); /* pointDistance, lib/common_lib.cpp:28-31 */
        if (range < lidarMinRange || range > lidarMaxRange) continue; /* :581-582 */
        int rowIdn = ring; /* :584 */
        if (rowIdn < 0 || rowIdn >= N_SCAN) continue; /* :585-586 */
        if (rowIdn % downsampleRate != 0) continue; /* :588-589 */
        if (i % point_filter_num != 0) continue; /* :591-592 */
        float q[4];
        deskew_point(&s, p, time, q); /* :594 */
        float *o = out + 8 * m++; /* :596 */
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = 0; o[4] = q[3]; o[5] = 0; o[6] = 0; o[7] = 0;
    }
    return m;
}
