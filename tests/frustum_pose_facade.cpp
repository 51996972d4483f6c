// Drives facade/FrameGeometry.h's FrustumPoseRow on a mock Frame built on cvcompat.h's Matx types: reads the bit patterns of 15 floats
// (mRcwx row-major, mtcwx, mOwx) from the command line, fills the members, and prints the bit patterns of tcwRow[12] and owRow[3].  Both
// overloads (members, Frame) are printed, one line each.  No device, no library: build with g++ alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../orb-slam3_amd/facade/FrameGeometry.h"

struct Frame {
    cv::Matx31f mOwx;
    cv::Matx33f mRcwx;
    cv::Matx31f mtcwx;
};

static float from_bits(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
static unsigned bits(float f) { unsigned b; std::memcpy(&b, &f, 4); return b; }

static void print(const float* t, const float* o) {
    for (int i = 0; i < 12; ++i) std::printf("%u ", bits(t[i]));
    for (int i = 0; i < 3; ++i) std::printf("%u%c", bits(o[i]), i == 2 ? '\n' : ' ');
}

int main(int argc, char** argv) {
    if (argc != 16) { std::fprintf(stderr, "usage: frustum_pose_facade R00 .. R22 t0 t1 t2 O0 O1 O2 (float bit patterns)\n"); return 2; }
    Frame F;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) F.mRcwx(r, c) = from_bits((unsigned)std::strtoul(argv[1 + 3 * r + c], nullptr, 10));
    for (int r = 0; r < 3; ++r) F.mtcwx(r) = from_bits((unsigned)std::strtoul(argv[10 + r], nullptr, 10));
    for (int r = 0; r < 3; ++r) F.mOwx(r) = from_bits((unsigned)std::strtoul(argv[13 + r], nullptr, 10));
    float t[12], o[3];
    for (float& x : t) x = -777.25f;
    for (float& x : o) x = -777.25f;
    ORB_SLAM3::FrustumPoseRow(F.mRcwx, F.mtcwx, F.mOwx, t, o);
    print(t, o);
    for (float& x : t) x = -777.25f;
    for (float& x : o) x = -777.25f;
    ORB_SLAM3::FrustumPoseRow(F, t, o);
    print(t, o);
    return 0;
}
