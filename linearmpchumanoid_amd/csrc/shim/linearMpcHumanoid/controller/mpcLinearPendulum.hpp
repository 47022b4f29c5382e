#pragma once
#include <Eigen/Dense>
#include <memory>
// LIPM preview controller (reference controller/mpcLinearPendulum.hpp:5-31): parameters, the last references, and compute() on its own.
// Inside Controller::standStep the preview step is evaluated by the GPU controller kernel and arrives through setRefs; a caller that uses
// the class alone gets the same step from lmh_mpc_step on a one-robot handle the object creates at its first compute().
class Mpc3dLip {
public:
    Mpc3dLip() {}
    Mpc3dLip(const double dt, const double timeHorizon, const double zCoM) : dt_(dt), timeHorizon_(timeHorizon), zCom_(zCoM) {}
    Mpc3dLip(const double dt, const double timeHorizon, const double zCoM, const double alpha, const double beta)
        : dt_(dt), timeHorizon_(timeHorizon), zCom_(zCoM), alpha_(alpha), beta_(beta) {}
    Eigen::Vector3d getXRef() const { return xRef_; }
    Eigen::Vector3d getYRef() const { return yRef_; }
    double getZCom() const { return zCom_; }
    double getDt() const { return dt_; }
    double getTimeHorizon() const { return timeHorizon_; }
    double getAlpha() const { return alpha_; }
    double getBeta() const { return beta_; }
    void setRefs(const double *x3, const double *y3) { for (int i = 0; i < 3; i++) { xRef_(i) = x3[i]; yRef_(i) = y3[i]; } }
    // src/mpcLinearPendulum.cpp:78-109: k = int(t / dt), u0 = first entry of -H^-1 g on zmp[k .. k + N], xRef = (A x + B u0, u0)
    void compute(const Eigen::Vector2d &posCom, const Eigen::Vector2d &velCom, const Eigen::VectorXd &zmpXRef, const Eigen::VectorXd &zmpYRef, double t);
private:
    Eigen::Vector3d xRef_, yRef_;
    double dt_ = 0.01, timeHorizon_ = 0.5, zCom_ = 0.26, alpha_ = 1e-3, beta_ = 1;
    struct Device;                        // the one-robot handle and the copy of the arrays it holds (lmh_shim.cpp); copies of the object share it
    std::shared_ptr<Device> dev_;
};
