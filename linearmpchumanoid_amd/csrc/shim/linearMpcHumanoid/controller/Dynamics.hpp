#pragma once
#include <Eigen/Dense>
#include "linearMpcHumanoid/robotInfo/Robot.hpp"
// Same call surface as the reference's controller/Dynamics.hpp: computeAll(robot) evaluates every term for the Robot's q and its stored
// velocity v_ (Robot::getJointsVelocity) in ONE lmh_terms_host call on the GPU; the getters hand out what that call returned, in the
// reference's shapes: M 30 x 30, C 30, Cg 30 (entries 0..5 carry values, the kernels form only those; the rest is zero), AG 6 x 30,
// AGpqp 6, Jpqp 12.  Every velocity product is taken at that one v_.
class Dynamics {
public:
    Dynamics() = default;
    void computeAll(const Robot &robot);
    const Eigen::VectorXd &getC() const { return C_; }
    const Eigen::VectorXd &getCg() const { return Cg_; }
    const Eigen::MatrixXd &getM() const { return M_; }
    const Eigen::MatrixXd &getAG() const { return AG_; }
    const Eigen::VectorXd &getAGpqp() const { return AGpqp_; }
    const Eigen::VectorXd &getJpqp() const { return Jpqp_; }
private:
    Eigen::VectorXd C_, Cg_, AGpqp_, Jpqp_;
    Eigen::MatrixXd M_, AG_;
};
